from mimo_unet_amd.evaluation import (UncertaintyEvaluator, cutoff_indices, standard_quantiles,  # noqa: F401
                                     write_tables_csv)
