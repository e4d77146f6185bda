from syntalker_amd.tmr import ActorAgnosticEncoder  # noqa: F401
