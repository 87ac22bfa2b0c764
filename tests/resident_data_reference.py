"""numpy restatement of the resident data path's definitions, shared by test_resident_data_cpu.py / _gpu.py.

* `gather` — the definition of `mimo_dataset_gather` in include/mimo_hip.h.
* `getitem` / `collate` — the reference's ``NYUv2DepthDataset.__getitem__`` (mimo/datasets/nyuv2.py:38-53: index through
  ``shuffle_permutation``, ``label / 255.0`` and, with ``normalize``, ``image / 255.0`` in float64, ``torch.tensor(...)
  .permute(2, 0, 1).float()``) followed by the DataLoader's default collate (a stack along a new first axis).

The reference's own module cannot be imported where the tests run — it imports ``h5py`` at the top, which is not
installed — so nothing here is generated from it and no fixture is: these few lines are written from its text."""
import numpy as np


def table(divisor):
    """What a byte becomes: the float64 quotient rounded once to fp32, or the byte itself."""
    ramp = np.arange(256)
    return (ramp if divisor is None else ramp / divisor).astype(np.float32)


def gather(fields, index, remap, n_samples):
    """fields: list of (src uint8 [n_samples,H,W,c], lut float32 [256]); returns a list of float32 [B,c,H,W]."""
    i = np.clip(np.asarray(index, dtype=np.int64), 0, n_samples - 1)
    j = i if remap is None else np.clip(np.asarray(remap, dtype=np.int64)[i], 0, n_samples - 1)
    return [np.ascontiguousarray(lut[src[j]].transpose(0, 3, 1, 2)) for src, lut in fields]


def getitem(image_u8, depth_u8, shuffle_permutation, normalize, index):
    s = shuffle_permutation[index]
    image, label = image_u8[s], depth_u8[s] / 255.0
    if normalize:
        image = image / 255.0
    return {"image": image.transpose(2, 0, 1).astype(np.float32), "label": label.transpose(2, 0, 1).astype(np.float32)}


def collate(image_u8, depth_u8, shuffle_permutation, normalize, indices):
    items = [getitem(image_u8, depth_u8, shuffle_permutation, normalize, int(i)) for i in indices]
    return {k: np.stack([it[k] for it in items]) for k in ("image", "label")}


def arrays(n, h, w, ci, seed):
    """Seeded uint8 image [n,h,w,ci] and depth [n,h,w,1] that hold every byte value (when they have 256 bytes or more)."""
    rng = np.random.RandomState(seed)
    image = rng.randint(0, 256, size=(n, h, w, ci)).astype(np.uint8)
    depth = rng.randint(0, 256, size=(n, h, w, 1)).astype(np.uint8)
    flat = image.reshape(-1)
    flat[:min(256, flat.size)] = np.arange(min(256, flat.size), dtype=np.uint8)
    return image, depth
