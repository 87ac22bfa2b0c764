"""Host side of the resident data path (no GPU): the normalisation table, the dataset against the restated reference,
the epoch order, the data module's interface and route choice, the new entry point's declaration, and the imports of the
reference's scripts/train/train_nyuv2_depth.py."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import resident_data_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_is_the_rounded_float64_quotient():
    from mimo_unet_amd.data import normalisation_table
    t = normalisation_table(255.0)
    assert t.dtype == np.float32 and t.shape == (256,)
    assert np.array_equal(t, (np.arange(256) / 255.0).astype(np.float32))
    # ... and is what the restated __getitem__ makes of every byte value
    image = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    item = R.getitem(image, image, np.arange(1), True, 0)
    assert np.array_equal(item["image"].reshape(-1), t) and np.array_equal(item["label"].reshape(-1), t)
    assert np.array_equal(normalisation_table(None), np.arange(256, dtype=np.float32))
    # why the kernel looks up and does not multiply by a reciprocal
    assert int((np.arange(256, dtype=np.float32) * np.float32(1 / 255.0) != t).sum()) == 126


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shuffle_on_load,use_fraction", [(False, 1.0), (True, 1.0), (False, 0.5), (True, 0.5)])
def test_dataset_from_arrays_equals_the_restatement(normalize, shuffle_on_load, use_fraction):
    from mimo.datasets.nyuv2 import NYUv2DepthDataset
    image, depth = R.arrays(9, 5, 7, 3, seed=3)
    np.random.seed(11)
    ds = NYUv2DepthDataset.from_arrays(image, depth, normalize=normalize, shuffle_on_load=shuffle_on_load,
                                       use_fraction=use_fraction)
    # the reference's draws, in its order (nyuv2.py:27-36)
    np.random.seed(11)
    perm = np.random.permutation(9) if shuffle_on_load else np.arange(9)
    if use_fraction < 1.0:
        perm = np.random.choice(perm, size=int(9 * use_fraction), replace=False)
    assert len(ds) == len(perm) == (9 if use_fraction == 1.0 else 4)
    assert np.array_equal(ds.shuffle_permutation, perm)
    for i in range(len(ds)):
        got, want = ds[i], R.getitem(image, depth, perm, normalize, i)
        assert set(got) == {"image", "label"}
        for k in want:
            assert got[k].dtype == torch.float32 and tuple(got[k].shape) == want[k].shape
            assert np.array_equal(got[k].numpy(), want[k]), (k, i)
    assert np.array_equal(NYUv2DepthDataset.depth_to_disparity(np.array([0.25, 1.0])), np.array([0.75, 0.0]))
    fields, remap = ds.resident_fields()
    assert fields["image"][1] == (255.0 if normalize else None) and fields["label"][1] == 255.0 and remap is ds.shuffle_permutation
    with pytest.raises(ValueError):
        NYUv2DepthDataset.from_arrays(image, depth[:, :4])


def test_default_collate_of_the_dataset_equals_the_restated_collate():
    from mimo.datasets.nyuv2 import NYUv2DepthDataset
    image, depth = R.arrays(6, 4, 6, 3, seed=4)
    np.random.seed(5)
    ds = NYUv2DepthDataset.from_arrays(image, depth, shuffle_on_load=True)
    batches = list(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, drop_last=False))
    assert [len(b["image"]) for b in batches] == [4, 2]
    for k, b in enumerate(batches):
        want = R.collate(image, depth, ds.shuffle_permutation, True, range(4 * k, min(6, 4 * k + 4)))
        assert all(np.array_equal(b[name].numpy(), want[name]) for name in want)


def test_epoch_indices():
    from mimo_unet_amd.data import epoch_indices
    a = epoch_indices(10, 0, True, seed=3)
    assert a.dtype == torch.int64 and sorted(a.tolist()) == list(range(10))
    assert torch.equal(a, epoch_indices(10, 0, True, seed=3))
    assert not torch.equal(a, epoch_indices(10, 1, True, seed=3))
    assert torch.equal(epoch_indices(10, 1, True, seed=3), epoch_indices(10, 0, True, seed=4))  # seed + epoch
    assert torch.equal(epoch_indices(10, 5, False), torch.arange(10))
    # every rank draws the same permutation and takes a strided share of it
    shares = [epoch_indices(10, 2, True, seed=3, rank=r, world_size=3) for r in range(3)]
    full = epoch_indices(10, 2, True, seed=3)
    for r, s in enumerate(shares):
        assert torch.equal(s, full[r::3])
    assert [len(s) for s in shares] == [4, 3, 3]
    assert sorted(torch.cat(shares).tolist()) == list(range(10))
    with pytest.raises(ValueError):
        epoch_indices(10, 0, True, rank=3, world_size=3)


def test_loader_length_arithmetic():
    from mimo_unet_amd.data import ResidentLoader

    class Ten:
        def __len__(self):
            return 10

    assert len(ResidentLoader(Ten(), 4, drop_last=True)) == 2
    assert len(ResidentLoader(Ten(), 4, drop_last=False)) == 3
    assert len(ResidentLoader(Ten(), 5, drop_last=False)) == 2
    assert len(ResidentLoader(Ten(), 4, drop_last=False, rank=1, world_size=3)) == 1  # a share of 3
    assert len(ResidentLoader(Ten(), 4, drop_last=True, rank=1, world_size=3)) == 0
    with pytest.raises(ValueError):
        ResidentLoader(Ten(), 0)


def test_datamodule_argparse_group_is_the_reference_s(tmp_path):
    from mimo.tasks.depth.nyuv2_datamodule import NYUv2DepthDataModule
    parser = NYUv2DepthDataModule.add_model_specific_args(argparse.ArgumentParser())
    group = [g for g in parser._action_groups if g.title == "NYUv2DepthDataModule"]
    assert len(group) == 1
    options = {a.dest: a for a in group[0]._group_actions}
    # nyuv2_datamodule.py:96-128
    assert {k: (a.type.__name__, a.default) for k, a in options.items()} == {
        "dataset_dir": ("dir_path", "/scratch/datasets/sen12tp-cropland-splitted/"), "batch_size": ("int", 32),
        "num_workers": ("int", 32), "pin_memory": ("bool", True), "train_dataset_fraction": ("float", 1.0)}
    args = parser.parse_args(["--dataset_dir", str(tmp_path), "--batch_size", "8", "--train_dataset_fraction", "0.5"])
    dm = NYUv2DepthDataModule.from_args(args)
    assert (str(dm.dataset_dir), dm.batch_size, dm.num_workers, dm.pin_memory, dm.normalize, dm.train_dataset_fraction) == \
        (str(tmp_path), 8, 32, True, True, 0.5)
    assert dm.resident is None and dm.resident_max_fraction == 0.25
    import inspect
    names = list(inspect.signature(NYUv2DepthDataModule.__init__).parameters)
    assert names[:7] == ["self", "dataset_dir", "batch_size", "num_workers", "pin_memory", "normalize", "train_dataset_fraction"]


def test_datamodule_resident_false_yields_dataloaders(monkeypatch, caplog):
    import mimo_unet_amd.tasks.depth.nyuv2_datamodule as D
    from mimo_unet_amd.datasets.nyuv2 import NYUv2DepthDataset
    image, depth = R.arrays(10, 4, 6, 3, seed=6)
    opened = []

    def from_file(dataset_path, **kwargs):  # stands in for the h5 file
        opened.append((os.path.basename(dataset_path), kwargs))
        return NYUv2DepthDataset.from_arrays(image, depth, **kwargs)

    monkeypatch.setattr(D, "NYUv2DepthDataset", from_file)
    dm = D.NYUv2DepthDataModule("/data", batch_size=4, num_workers=0, pin_memory=False, train_dataset_fraction=0.5,
                                resident=False)
    with caplog.at_level("INFO", logger=D.__name__):
        np.random.seed(0)
        dm.setup()
    # nyuv2_datamodule.py:33-50
    assert opened == [("depth_train.h5", dict(normalize=True, shuffle_on_load=False, use_fraction=0.5)),
                      ("depth_train.h5", dict(normalize=True, shuffle_on_load=True)),
                      ("depth_test.h5", dict(normalize=True, shuffle_on_load=True))]
    assert "DataLoader route: resident=False" in caplog.text
    loaders = dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()
    assert all(type(ld) is torch.utils.data.DataLoader for ld in loaders)
    assert [ld.drop_last for ld in loaders] == [True, False, False]
    assert [type(ld.sampler).__name__ for ld in loaders] == ["RandomSampler", "SequentialSampler", "SequentialSampler"]
    assert [len(ld) for ld in loaders] == [1, 3, 3]  # 5 // 4, ceil(10 / 4)
    batch = next(iter(loaders[1]))
    want = R.collate(image, depth, dm.data_valid.shuffle_permutation, True, range(4))
    assert all(np.array_equal(batch[k].numpy(), want[k]) for k in want)
    if not torch.cuda.is_available():
        dm.resident = None  # automatic, and no GPU is visible
        with caplog.at_level("INFO", logger=D.__name__):
            dm._choose_route()
        assert "DataLoader route: no GPU is visible" in caplog.text and dm.resident_sets is None
        dm.resident = True
        with pytest.raises(RuntimeError):
            dm._choose_route()


def test_lightning_datamodule_base_is_exported():
    from mimo_unet_amd import lightning_compat as L
    from mimo.tasks.depth.nyuv2_datamodule import NYUv2DepthDataModule
    assert issubclass(NYUv2DepthDataModule, L.LightningDataModule)
    for hook in ("prepare_data", "setup", "teardown"):
        assert callable(getattr(L.LightningDataModule, hook))


def test_entry_point_is_declared_and_exported(built_library):
    import ctypes as C
    from mimo_unet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    assert re.search(r"\bint mimo_dataset_gather\s*\(", header) and "typedef struct mimo_gather_field" in header
    assert re.search(r"global:\s*mimo_\*;", open(os.path.join(ROOT, "mimo_unet_amd", "csrc", "exports.map")).read())
    assert "mimo_dataset_gather" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "mimo_dataset_gather")
    assert "dataset_gather.hip" in open(os.path.join(ROOT, "Makefile")).read()
    assert C.sizeof(_lib.GatherField) == 32 and _lib.GatherField.dst.offset == 16 and _lib.GatherField.c.offset == 24
    # refused before anything touches a device: no fields, a null table
    assert lib.mimo_dataset_gather(None, 0, None, None, 1, 1, 1, 1, None) == -1
    assert b"0 fields" in lib.mimo_last_error()
    assert lib.mimo_dataset_gather(None, 1, None, None, 1, 1, 1, 1, None) == -1


def test_train_script_imports_resolve():
    """scripts/train/train_nyuv2_depth.py:12-15 of the reference."""
    from mimo.utils import dir_path  # noqa: F401
    from mimo.models.mimo_unet import MimoUnetModel  # noqa: F401
    from mimo.tasks.depth.nyuv2_datamodule import NYUv2DepthDataModule
    from mimo.tasks.depth.callbacks import OutputMonitor, WandbMetricsDefiner
    import mimo.datasets.nyuv2 as A
    import mimo.monitor
    import mimo_unet_amd.datasets.nyuv2 as M
    import mimo_unet_amd.tasks.depth.nyuv2_datamodule as D
    assert A.NYUv2DepthDataset is M.NYUv2DepthDataset and NYUv2DepthDataModule is D.NYUv2DepthDataModule
    assert OutputMonitor is mimo.monitor.OutputMonitor
    OutputMonitor()  # train_nyuv2_depth.py:23 constructs it without arguments
    import mimo.tasks.depth.callbacks as CB
    assert WandbMetricsDefiner.SUMMARIES == {"metric_val/r2": "max", "metric_val/mae": "min", "metric_val/mse": "min"}
    if CB.wandb is None:
        WandbMetricsDefiner().on_fit_start(None, None)  # a no-op without wandb
