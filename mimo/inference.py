from mimo_unet_amd.inference import SceneTiler, predict_scene  # noqa: F401
