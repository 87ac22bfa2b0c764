"""The resident data path on the GPU: `mimo_dataset_gather` bit for bit against its numpy restatement
(tests/resident_data_reference.py) at the smallest shapes where it can go wrong, its argument checks, `ResidentLoader`
against the restated ``__getitem__`` + collate, the data module's resident route, and one training step on a resident
batch against the same batch built on the host.

Shapes: 5 x 7 and 15 x 21 (h * w % 4 != 0: byte loads, a tail of 3 pixels per sample, destination planes off the 16-byte
grid; the second with more than one workgroup), 8 x 8 and 24 x 40 (dword loads, float4 stores; the second with more than
one workgroup), 4 x 6 with the source one byte into its allocation (byte loads on a shape that is otherwise read in dwords)
and with the destination one float into its allocation (scalar stores on a shape that is otherwise written as float4)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import resident_data_reference as R

pytestmark = pytest.mark.gpu

N = 7  # samples in the store of the kernel cases
GUARD, SENTINEL = 64, -7.0
REMAPS = {"none": None, "permutation": [3, 0, 6, 1, 5, 2, 4], "out_of_range": [9, -2, 6, 1, 1 << 40, 2, -(1 << 40)]}
INDICES = {1: [N - 1], 5: [N - 1, 2, 2, -1, N + 3]}  # the last sample, a repeat, and two indices the clamp brings back


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Field:
    """A source (optionally `src_shift` bytes into a larger allocation), its table, and a sentinel-filled destination with
    guard floats on both sides (optionally `dst_shift` floats further in)."""

    def __init__(self, src, divisor, batch, src_shift=0, dst_shift=0):
        self.src, self.lut = src, R.table(divisor)
        n, h, w, c = src.shape
        self.store = torch.zeros(src.size + src_shift + 3, dtype=torch.uint8, device="cuda")
        self.store[src_shift:src_shift + src.size] = _dev(src.reshape(-1))
        self.src_ptr = self.store.data_ptr() + src_shift
        self.lut_dev = _dev(self.lut)
        self.shape = (batch, c, h, w)
        self.numel = batch * c * h * w
        self.buf = torch.full((GUARD + dst_shift + self.numel + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.first = GUARD + dst_shift
        self.dst_ptr = self.buf.data_ptr() + 4 * self.first
        self.c = c

    def out(self):
        return self.buf[self.first:self.first + self.numel].view(self.shape).cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:self.first] == SENTINEL).all() and (b[self.first + self.numel:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _call(fields, index, remap, n_samples, batch, h, w, n_fields=None, raw=None):
    from mimo_unet_amd import _lib
    table = (_lib.GatherField * max(len(fields), 1))(*(
        _lib.GatherField(*(raw[i] if raw and i in raw else (f.src_ptr, f.lut_dev.data_ptr(), f.dst_ptr, f.c)), 0)
        for i, f in enumerate(fields)))
    rc = _lib.load().mimo_dataset_gather(table, len(fields) if n_fields is None else n_fields, _lib.ptr(index),
                                         _lib.ptr(remap), n_samples, batch, h, w, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


CASES = {
    # name: (h, w, [(channels, divisor, src_shift, dst_shift)])
    "5x7_bytes_tail": (5, 7, [(3, 255.0, 0, 0), (1, None, 0, 0)]),
    "15x21_bytes_tail_blocks": (15, 21, [(3, 255.0, 0, 0), (1, 255.0, 0, 0)]),
    "8x8_dwords": (8, 8, [(1, 255.0, 0, 0), (2, None, 0, 0), (3, 100.0, 0, 0), (4, 255.0, 0, 0)]),
    "24x40_dwords_blocks": (24, 40, [(3, 255.0, 0, 0), (1, 255.0, 0, 0)]),
    "4x6_source_off_by_one_byte": (4, 6, [(3, 255.0, 1, 0), (1, 255.0, 0, 0)]),
    "4x6_destination_off_by_one_float": (4, 6, [(3, 255.0, 0, 1), (1, None, 2, 3)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gather_equals_the_definition(case):
    h, w, spec = CASES[case]
    sources = [R.arrays(N, h, w, c, seed=20 + k)[0] for k, (c, _, _, _) in enumerate(spec)]
    for batch, index in INDICES.items():
        for name, remap in REMAPS.items():
            fields = [_Field(src, div, batch, s_shift, d_shift) for src, (_, div, s_shift, d_shift) in zip(sources, spec)]
            idx = torch.tensor(index, dtype=torch.int64, device="cuda")
            rm = None if remap is None else torch.tensor(remap, dtype=torch.int64, device="cuda")
            assert _call(fields, idx, rm, N, batch, h, w) == 0
            want = R.gather([(f.src, f.lut) for f in fields], index, remap, N)
            for k, f in enumerate(fields):
                got = f.out()
                assert got.dtype == np.float32 and np.array_equal(got, want[k]), (case, batch, name, k)
                assert f.guards_intact(), (case, batch, name, k)
            if remap is None:  # the clamp: rows of samples 0 and N - 1
                assert np.array_equal(want[0][-1 if batch == 5 else 0], fields[0].lut[sources[0][N - 1]].transpose(2, 0, 1))
                if batch == 5:
                    assert np.array_equal(fields[0].out()[3], fields[0].lut[sources[0][0]].transpose(2, 0, 1))


def test_refused_arguments_launch_nothing():
    from mimo_unet_amd import _lib
    h, w, batch = 4, 6, 2
    image, depth = R.arrays(N, h, w, 3, seed=1)

    def fresh(n=2):
        return [_Field(image, 255.0, batch), _Field(depth, 255.0, batch)][:n]

    idx = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    good = fresh()
    assert _call(good, idx, None, N, batch, h, w) == 0 and not good[0].untouched()  # the call the refused ones are variations of

    def refused(what, fields, *args, **kw):
        rc = _call(fields, *args, **kw)
        assert rc != 0, what
        assert _lib.load().mimo_last_error().startswith(b"mimo_dataset_gather"), what
        assert all(f.untouched() for f in fields), what

    refused("no fields", fresh(), idx, None, N, batch, h, w, n_fields=0)
    refused("five fields", fresh() + fresh() + fresh(1), idx, None, N, batch, h, w)
    refused("null index", fresh(), None, None, N, batch, h, w)
    for bad_c in (0, 5, -1):
        f = fresh()
        refused(f"c = {bad_c}", f, idx, None, N, batch, h, w, raw={1: (f[1].src_ptr, f[1].lut_dev.data_ptr(), f[1].dst_ptr, bad_c)})
    f = fresh()
    refused("null src", f, idx, None, N, batch, h, w, raw={0: (None, f[0].lut_dev.data_ptr(), f[0].dst_ptr, 3)})
    f = fresh()
    refused("null lut", f, idx, None, N, batch, h, w, raw={1: (f[1].src_ptr, None, f[1].dst_ptr, 1)})
    f = fresh()
    refused("null dst", f, idx, None, N, batch, h, w, raw={1: (f[1].src_ptr, f[1].lut_dev.data_ptr(), None, 1)})
    refused("batch 0", fresh(), idx, None, N, 0, h, w)
    refused("h 0", fresh(), idx, None, N, batch, 0, w)
    refused("w 0", fresh(), idx, None, N, batch, h, 0)
    refused("w < 0", fresh(), idx, None, N, batch, h, -6)
    refused("no samples", fresh(), idx, None, 0, batch, h, w)
    refused("a batch of 2^31 elements", fresh(), idx, None, N, 1 << 11, 1 << 9, 1 << 9)
    refused("a store of more than 2^62 bytes", fresh(), idx, None, 1 << 58, batch, h, w)
    # ... and a null field table
    assert _lib.load().mimo_dataset_gather(None, 2, idx.data_ptr(), None, N, batch, h, w, _lib.current_stream()) != 0


def _dataset(n, h, w, **kwargs):
    from mimo.datasets.nyuv2 import NYUv2DepthDataset
    image, depth = R.arrays(n, h, w, 3, seed=9)
    np.random.seed(2)
    return image, depth, NYUv2DepthDataset.from_arrays(image, depth, **kwargs)


@pytest.mark.parametrize("kwargs,drop_last", [(dict(shuffle_on_load=True), False), (dict(normalize=False), False),
                                              (dict(shuffle_on_load=True, use_fraction=0.5), True)])
def test_loader_yields_the_collated_batches_in_epoch_order(kwargs, drop_last):
    from mimo_unet_amd.data import ResidentDataset, ResidentLoader, epoch_indices
    image, depth, ds = _dataset(10, 5, 7, **kwargs)
    store = ResidentDataset(*ds.resident_fields())
    assert len(store) == len(ds) and (store.remap is None) == (len(ds) != 10)  # a shorter remap selects on the host
    loader = ResidentLoader(store, batch_size=4, shuffle=True, drop_last=drop_last, seed=5)
    epochs = []
    for epoch in range(2):
        order = epoch_indices(len(ds), epoch, True, seed=5).tolist()
        batches = list(loader)  # no set_epoch: the loader advances by itself
        sizes = [4] * (len(ds) // 4) + ([len(ds) % 4] if len(ds) % 4 and not drop_last else [])
        assert len(batches) == len(loader) == len(sizes)
        for k, b in enumerate(batches):
            want = R.collate(image, depth, ds.shuffle_permutation, ds.normalize, order[4 * k:4 * k + sizes[k]])
            assert set(b) == {"image", "label"}
            for name in want:
                assert b[name].is_cuda and b[name].dtype == torch.float32 and b[name].is_contiguous()
                assert np.array_equal(b[name].cpu().numpy(), want[name]), (epoch, k, name)
        epochs.append(batches)
    assert not torch.equal(epochs[0][0]["image"], epochs[1][0]["image"])
    # the same seed replays the same epoch: a second loader, and this one put back to epoch 0
    again = list(ResidentLoader(store, batch_size=4, shuffle=True, drop_last=drop_last, seed=5))
    loader.set_epoch(0)
    replay = list(loader)
    for a, b, c in zip(epochs[0], again, replay):
        assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a)
    # fresh tensors per batch: nothing a later batch overwrites
    assert len({b["image"].data_ptr() for b in epochs[0]}) == len(epochs[0])


def test_loader_shares_of_two_ranks_cover_the_epoch():
    from mimo_unet_amd.data import ResidentDataset, ResidentLoader
    image, depth, ds = _dataset(10, 4, 6)
    store = ResidentDataset(*ds.resident_fields())
    labels = [torch.cat([b["label"] for b in ResidentLoader(store, 2, shuffle=True, seed=1, rank=r, world_size=2)])
              for r in range(2)]
    whole = torch.cat([b["label"] for b in ResidentLoader(store, 10, shuffle=True, seed=1)])
    assert torch.equal(whole[0::2], labels[0]) and torch.equal(whole[1::2], labels[1])


def test_gather_refuses_a_host_index():
    from mimo_unet_amd.data import ResidentDataset
    _, _, ds = _dataset(4, 4, 6)
    store = ResidentDataset(*ds.resident_fields())
    with pytest.raises(ValueError):
        store.gather(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        store.gather(torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert store.gather(torch.zeros(0, dtype=torch.int64, device="cuda"))["image"].shape == (0, 3, 4, 6)


def test_datamodule_takes_the_resident_route(monkeypatch, caplog):
    import mimo_unet_amd.tasks.depth.nyuv2_datamodule as D
    from mimo_unet_amd.data import ResidentLoader
    from mimo_unet_amd.datasets.nyuv2 import NYUv2DepthDataset
    image, depth = R.arrays(10, 4, 6, 3, seed=6)
    monkeypatch.setattr(D, "NYUv2DepthDataset", lambda path, **kw: NYUv2DepthDataset.from_arrays(image, depth, **kw))
    dm = D.NYUv2DepthDataModule("/data", batch_size=4, num_workers=0, pin_memory=False, train_dataset_fraction=0.5)
    with caplog.at_level("INFO", logger=D.__name__):
        np.random.seed(0)
        dm.setup()
    assert "resident route: the stores take" in caplog.text
    loaders = dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()
    assert all(isinstance(ld, ResidentLoader) for ld in loaders)
    assert [(ld.shuffle, ld.drop_last, len(ld)) for ld in loaders] == [(True, True, 1), (False, False, 3), (False, False, 3)]
    for k, b in enumerate(loaders[1]):
        want = R.collate(image, depth, dm.data_valid.shuffle_permutation, True, range(4 * k, min(10, 4 * k + 4)))
        assert all(np.array_equal(b[name].cpu().numpy(), want[name]) for name in want)
    # a budget the stores do not fit in: the reference's route, and the log says why
    dm.resident_max_fraction = 0.0
    with caplog.at_level("INFO", logger=D.__name__):
        dm._choose_route()
    assert "DataLoader route: the stores would take" in caplog.text
    assert type(dm.train_dataloader()) is torch.utils.data.DataLoader


def test_training_step_on_a_resident_batch_equals_the_host_batch():
    """f = 4, S = 2, batch 4 at 32 x 32: the smallest image the engine plans (at 16 x 16 mimo_plan_create refuses — the
    reflect padding needs 2 pixels at 1/16 resolution)."""
    from mimo.models.mimo_unet import MimoUnetModel
    from mimo_unet_amd.data import ResidentDataset, ResidentLoader
    image, depth, ds = _dataset(8, 32, 32, shuffle_on_load=True)
    host = next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)))
    resident = next(iter(ResidentLoader(ResidentDataset(*ds.resident_fields()), batch_size=4, shuffle=False)))
    losses = []
    for batch in ({k: v.cuda() for k, v in host.items()}, resident):
        torch.manual_seed(0)
        model = MimoUnetModel(in_channels=3, out_channels=2, num_subnetworks=2, filter_base_count=4, center_dropout_rate=0.0,
                              final_dropout_rate=0.0, encoder_dropout_rate=0.0, core_dropout_rate=0.0,
                              decoder_dropout_rate=0.0, loss="laplace_nll", weight_decay=0.0, learning_rate=1e-3, seed=0,
                              loss_buffer_size=10, loss_buffer_temperature=0.3).cuda().train()
        torch.manual_seed(11)  # the permutation streams
        losses.append(model.training_step(batch, 0)["loss"].detach().cpu())
    assert all(torch.equal(host[k].cuda(), resident[k]) for k in host)
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])
