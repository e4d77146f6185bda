from syntalker_amd.metrics import L1div, alignment  # noqa: F401
