from mimo_unet_amd.datasets.nyuv2 import NYUv2DepthDataset  # noqa: F401
