from mimo_unet_amd.adversarial import (DEFAULT_EPSILONS, RobustnessEvaluator, fgsm_sweep, image_gradient, pgd_sweep)  # noqa: F401
