from mimo_unet_amd.evaluation import (SOURCES, UncertaintyEvaluator, check_sources, cutoff_indices,  # noqa: F401
                                     sparsification_areas, standard_quantiles, write_sparsification_csv, write_tables_csv)
