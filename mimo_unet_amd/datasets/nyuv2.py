"""The reference's NYUv2 depth dataset (``mimo/datasets/nyuv2.py:7-60``): uint8 images ``[N,H,W,3]`` and uint8 depth
``[N,H,W,1]`` from one h5 file, served per sample as fp32 CHW tensors in [0, 1].

Same constructor, ``__getitem__``, ``__len__`` and ``depth_to_disparity``, and the same draws from ``np.random`` in the
same order (``shuffle_on_load`` first, then ``use_fraction``), so a run seeded with ``seed_everything`` selects the same
samples.  ``h5py`` is imported by the constructor only; `from_arrays` builds the dataset from arrays already in memory.
The arrays stay uint8: `mimo_unet_amd.data.ResidentDataset` uploads them as they are (`resident_fields`)."""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import Dataset


class NYUv2DepthDataset(Dataset):
    """The label is a scaled depth map (near: 0 - far: 1)."""

    def __init__(self, dataset_path: str, normalize: bool = True, shuffle_on_load: bool = False,
                 use_fraction: float = 1.0) -> None:
        super().__init__()
        import h5py  # here and not at the top: the resident path, the tests and the measurements do not need it
        with h5py.File(dataset_path, "r") as h5_data:
            data = dict(image=np.array(h5_data["image"]), label=np.array(h5_data["depth"]))
        self._init(data, normalize, shuffle_on_load, use_fraction)

    @classmethod
    def from_arrays(cls, image_u8, depth_u8, normalize: bool = True, shuffle_on_load: bool = False,
                    use_fraction: float = 1.0) -> "NYUv2DepthDataset":
        """The dataset over ``image_u8 [N,H,W,Ci]`` and ``depth_u8 [N,H,W,1]`` (what the h5 file holds), not copied."""
        image_u8, depth_u8 = np.asarray(image_u8), np.asarray(depth_u8)
        if image_u8.ndim != 4 or depth_u8.ndim != 4 or image_u8.shape[:3] != depth_u8.shape[:3]:
            raise ValueError(f"from_arrays: image {image_u8.shape} and depth {depth_u8.shape} must be [N,H,W,C] over the "
                             "same samples and pixels")
        self = cls.__new__(cls)
        Dataset.__init__(self)
        self._init(dict(image=image_u8, label=depth_u8), normalize, shuffle_on_load, use_fraction)
        return self

    def _init(self, data, normalize, shuffle_on_load, use_fraction) -> None:
        self.data = data
        self.normalize = normalize
        n = len(data["image"])
        self.shuffle_permutation = np.random.permutation(n) if shuffle_on_load else np.arange(n)
        if use_fraction < 1.0:
            self.num_items = int(n * use_fraction)
            self.shuffle_permutation = np.random.choice(self.shuffle_permutation, size=self.num_items, replace=False)
        else:
            self.num_items = n

    def __getitem__(self, index):
        shuffled_index = self.shuffle_permutation[index]
        image = self.data["image"][shuffled_index]
        label = self.data["label"][shuffled_index] / 255.0  # float64, rounded once by .float() below
        if self.normalize:
            image = image / 255.0
        return {
            "image": torch.tensor(image).permute(2, 0, 1).float(),
            "label": torch.tensor(label).permute(2, 0, 1).float(),
        }

    def __len__(self) -> int:
        return self.num_items

    @staticmethod
    def depth_to_disparity(depth_map: np.ndarray) -> np.ndarray:
        return 1 - depth_map

    def resident_fields(self):
        """``(fields, remap)`` for `mimo_unet_amd.data.ResidentDataset`: the byte arrays with the divisor `__getitem__`
        applies to each (None: the bytes as floats), and the sample order."""
        fields = {"image": (self.data["image"], 255.0 if self.normalize else None), "label": (self.data["label"], 255.0)}
        return fields, self.shuffle_permutation
