from mimo_unet_amd.adversarial import (DEFAULT_EPSILONS, RobustnessEvaluator, fgsm_sweep, image_gradient)  # noqa: F401
