from mimo_unet_amd.evaluation import (SOURCES, UncertaintyEvaluator, check_sources, cutoff_indices,  # noqa: F401
                                     sparsification_areas, standard_quantiles, write_sparsification_csv, write_tables_csv)
from mimo_unet_amd.evaluation import (MAX_MEMBERS, REGISTER_MEMBERS, SCORE_MAX_WORKGROUPS, PredictiveScorer, check_expected_p, check_score_shapes,  # noqa: F401
                                     check_evidential_score_shapes, coverage_table, mixture_of, write_scores_csv)
