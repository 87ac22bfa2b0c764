from mimo_unet_amd.tasks.depth.nyuv2_datamodule import NYUv2DepthDataModule  # noqa: F401
