"""Import-path shims: put ``syntalker_amd/dropin`` FIRST on sys.path (or call ``install()``) and the
reference's drivers (`train.py:85-94`, `diffusion_rvqvae_trainer.py:17-19,185`, `h3d_diffusion_new_trainer.py`)
pick up this implementation through their own import statements:

    from diffusion.model_util import create_gaussian_diffusion
    from diffusion.resample import create_named_schedule_sampler
    from diffusion.cfg_sampler import ClassifierFreeSampleModel, ...
    getattr(__import__("models.denoiser", fromlist=["something"]), "MDM")(args)

The reference's own ``models`` / ``diffusion`` packages contain much more than the hot path, so
``install()`` only overrides the five hot-path modules inside ``sys.modules`` and leaves the rest alone.
"""
import importlib
import sys

_MAP = {
    "diffusion.model_util": "syntalker_amd.dropin.diffusion.model_util",
    "diffusion.respace": "syntalker_amd.dropin.diffusion.respace",
    "diffusion.gaussian_diffusion": "syntalker_amd.dropin.diffusion.gaussian_diffusion",
    "diffusion.resample": "syntalker_amd.dropin.diffusion.resample",
    "diffusion.cfg_sampler": "syntalker_amd.dropin.diffusion.cfg_sampler",
    "models.denoiser": "syntalker_amd.dropin.models.denoiser",
    "models.denoiser_h3d": "syntalker_amd.dropin.models.denoiser_h3d",
}


# opt-in: the sampling / evaluation drivers only run the RVQ-VAEs in eval() (diffusion_rvqvae_trainer.py:28,105-161); the
# reference's RVQ-VAE *training* script needs the trainable original, so this alias is not installed by default
_MAP_RVQ = {"models.vq.model": "syntalker_amd.dropin.models.vq.model"}


# opt-in for the same reason: the reference's models/motion_representation.py also holds the VAE / VQ-VAE classes its other trainers train;
# this one carries the FGD evaluator (VAESKConv) only
_MAP_EVAL = {"models.motion_representation": "syntalker_amd.dropin.models.motion_representation"}


# opt-in: the reference's `utils` package holds far more than the T2M evaluator (h3d_diffusion_new_trainer.py imports its logging and
# rotation helpers from there); only `utils.t2m_eval_tools` - EvaluatorMDMWrapper and the evaluate_* metrics - is replaced
_MAP_T2M = {"utils.t2m_eval_tools": "syntalker_amd.dropin.utils.t2m_eval_tools"}


# opt-in, same package: `utils.metric` - L1div and alignment (beat consistency) on the device; the reference's SRGR, which nothing calls, is not in it
_MAP_METRIC = {"utils.metric": "syntalker_amd.dropin.utils.metric"}


def install(rvqvae: bool = False, evaluator: bool = False, t2m: bool = False, metric: bool = False):
    """Alias the hot-path modules under the reference's module names (rvqvae=True: also `models.vq.model.RVQVAE`; evaluator=True: also
    `models.motion_representation.VAESKConv`, the FGD evaluator; t2m=True: also `utils.t2m_eval_tools`, the h3d text-motion evaluator;
    metric=True: also `utils.metric`, L1div and the beat-consistency `alignment`)."""
    for ref_name, ours in {**_MAP, **(_MAP_RVQ if rvqvae else {}), **(_MAP_EVAL if evaluator else {}), **(_MAP_T2M if t2m else {}),
                           **(_MAP_METRIC if metric else {})}.items():
        mod = importlib.import_module(ours)
        sys.modules[ref_name] = mod
        parent, _, leaf = ref_name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, mod)
