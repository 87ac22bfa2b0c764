"""The reference's NYUv2 data module (``mimo/tasks/depth/nyuv2_datamodule.py:11-130``) with a second route for its three
loaders: the datasets resident in HBM and every batch gathered there (`mimo_unet_amd.data.ResidentLoader`).

Constructor, ``setup``, ``from_args`` and the argparse group are the reference's; the loaders keep its ``shuffle`` /
``drop_last`` per split.  ``resident`` chooses the route: ``False`` the reference's ``DataLoader`` over the host dataset,
``True`` the resident one, ``None`` (default) the resident one when a GPU is visible and the three byte stores fit in
``resident_max_fraction`` of the free device memory.  ``setup`` logs which route it took and why."""
from __future__ import annotations

import logging
import os
from argparse import ArgumentParser, Namespace
from typing import Optional

import torch

from ...data import ResidentDataset, ResidentLoader
from ...datasets.nyuv2 import NYUv2DepthDataset
from ...lightning_compat import LightningDataModule
from ...utils import dir_path

log = logging.getLogger(__name__)


class NYUv2DepthDataModule(LightningDataModule):
    def __init__(self, dataset_dir: str, batch_size: int, num_workers: int, pin_memory: bool, normalize: bool = True,
                 train_dataset_fraction: float = 1.0, resident: Optional[bool] = None,
                 resident_max_fraction: float = 0.25) -> None:
        super().__init__()
        self.dataset_dir = dataset_dir
        self.batch_size = batch_size
        self.num_workers = num_workers
        self.pin_memory = pin_memory
        self.normalize = normalize
        self.train_dataset_fraction = train_dataset_fraction
        self.resident = resident
        self.resident_max_fraction = resident_max_fraction
        self.resident_sets = None  # split -> ResidentDataset once setup() has chosen the resident route

    def setup(self, stage: Optional[str] = None) -> None:
        train_file = os.path.join(self.dataset_dir, "depth_train.h5")
        self.data_train = NYUv2DepthDataset(train_file, normalize=self.normalize, shuffle_on_load=False,
                                            use_fraction=self.train_dataset_fraction)
        self.data_valid = NYUv2DepthDataset(train_file, normalize=self.normalize, shuffle_on_load=True)
        self.data_test = NYUv2DepthDataset(os.path.join(self.dataset_dir, "depth_test.h5"), normalize=self.normalize,
                                           shuffle_on_load=True)
        self._choose_route()

    def _choose_route(self) -> None:
        """Decide between the two routes for the datasets `setup` made, say so in the log, upload for the resident one."""
        sets = {"train": self.data_train, "valid": self.data_valid, "test": self.data_test}
        use, why = self._decide(sum(_store_bytes(ds) for ds in sets.values()))
        log.info("NYUv2DepthDataModule: %s route: %s", "resident" if use else "DataLoader", why)
        self.resident_sets = None
        if use:
            self.resident_sets = {k: ResidentDataset(*ds.resident_fields()) for k, ds in sets.items()}

    def _decide(self, need: int):
        if self.resident is False:
            return False, "resident=False"
        if not torch.cuda.is_available():
            if self.resident:
                raise RuntimeError("NYUv2DepthDataModule(resident=True) needs a GPU and none is visible")
            return False, "no GPU is visible"
        if self.resident:
            return True, f"resident=True ({need / 2**20:.0f} MiB of bytes)"
        free, _ = torch.cuda.mem_get_info()
        room = int(free * self.resident_max_fraction)
        if need <= room:
            return True, f"the stores take {need / 2**20:.0f} MiB, {room / 2**20:.0f} MiB ({self.resident_max_fraction:g} of the free HBM) are allowed"
        return False, f"the stores would take {need / 2**20:.0f} MiB, above {room / 2**20:.0f} MiB ({self.resident_max_fraction:g} of the free HBM)"

    def _loader(self, split: str, dataset, shuffle: bool, drop_last: bool):
        if self.resident_sets is not None:
            rank, world_size = _rank_and_world_size(getattr(self, "trainer", None))
            # torch.initial_seed(): what seed_everything / torch.manual_seed set, so a seeded run replays its epochs
            return ResidentLoader(self.resident_sets[split], self.batch_size, shuffle=shuffle, drop_last=drop_last,
                                  seed=torch.initial_seed() % 2**31, rank=rank, world_size=world_size)
        return torch.utils.data.DataLoader(dataset, batch_size=self.batch_size, num_workers=self.num_workers, shuffle=shuffle,
                                           drop_last=drop_last, pin_memory=self.pin_memory)

    def train_dataloader(self):
        return self._loader("train", self.data_train, shuffle=True, drop_last=True)

    def val_dataloader(self):
        return self._loader("valid", self.data_valid, shuffle=False, drop_last=False)

    def test_dataloader(self):
        return self._loader("test", self.data_test, shuffle=False, drop_last=False)

    @classmethod
    def from_args(cls, args: Namespace) -> "NYUv2DepthDataModule":
        return cls(dataset_dir=args.dataset_dir, batch_size=args.batch_size, num_workers=args.num_workers,
                   pin_memory=args.pin_memory, train_dataset_fraction=args.train_dataset_fraction)

    @staticmethod
    def add_model_specific_args(parent_parser: ArgumentParser) -> ArgumentParser:
        parser = parent_parser.add_argument_group(title="NYUv2DepthDataModule")
        parser.add_argument("--dataset_dir", type=dir_path, default="/scratch/datasets/sen12tp-cropland-splitted/")
        parser.add_argument("--batch_size", type=int, default=32, help="Specify the batch size.")
        parser.add_argument("--num_workers", type=int, default=32, help="Specify the number of workers.")
        parser.add_argument("--pin_memory", type=bool, default=True, help="Specify whether to pin memory.")
        parser.add_argument("--train_dataset_fraction", type=float, default=1.0,
                            help="Specify the fraction of the training dataset to use.")
        return parent_parser


def _store_bytes(ds: NYUv2DepthDataset) -> int:
    """Bytes a `ResidentDataset` of this dataset uploads: all samples, or the selected ones under use_fraction < 1."""
    n = len(ds.data["image"])
    return sum(a.nbytes for a in ds.data.values()) // max(n, 1) * len(ds)


def _rank_and_world_size(trainer):
    if trainer is not None and hasattr(trainer, "global_rank"):
        return int(trainer.global_rank), int(trainer.world_size)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1
