from syntalker_amd.tmr import DistilbertActorAgnosticEncoder  # noqa: F401
