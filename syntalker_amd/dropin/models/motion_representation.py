from syntalker_amd.evaluator import VAESKConv  # noqa: F401
