from syntalker_amd.metrics import (calculate_activation_statistics, calculate_diversity, calculate_multimodality, calculate_top_k,  # noqa: F401
                                   euclidean_distance_matrix, evaluate_diversity, evaluate_fid, evaluate_matching_score,
                                   evaluate_multimodality, get_metric_statistics, t2m_frechet_distance as calculate_frechet_distance)
from syntalker_amd.t2m_evaluator import (EvaluatorMDMWrapper, MotionEncoderBiGRUCo, MovementConvEncoder, TextEncoderBiGRUCo,  # noqa: F401
                                         build_evaluators)
