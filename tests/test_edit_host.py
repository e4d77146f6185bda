"""In-painting on the fused sampling loop, without a GPU: the C ABI's `syn_edit` / `syn_denoise_step_edit` (struct mirror, symbol, refusals),
`longform.keep_mask` and the per-window slices of `sample_long(edit=...)`, which loop calls the fused path takes, and the property of the
blend the GPU tests rely on (an all-True mask returns `inpainted_motion` exactly)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from syntalker_amd import _lib, longform

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_c_abi_edit_struct_size_matches_the_ctypes_mirror():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "syn_hip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(syn_edit), '
                             'offsetof(syn_edit, keep), offsetof(syn_edit, known));return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SynEdit), _lib.SynEdit.keep.offset, _lib.SynEdit.known.offset] == [16, 0, 8]


def test_symbol_is_in_the_header_the_library_and_exports():
    assert "syn_denoise_step_edit" in _lib.EXPORTS
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert "int syn_denoise_step_edit(const syn_model* model, const syn_step* step, const syn_edit* edit, void* stream);" in header
    assert "#define SYN_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9           # additive: the version stays
    lib = _lib.load()
    assert lib.syn_denoise_step_edit.restype is ctypes.c_int
    assert lib.syn_denoise_step_edit.argtypes[2] is ctypes.POINTER(_lib.SynEdit)


def test_step_edit_refusals_name_the_cause():
    """Each refusal happens before any launch (no GPU here): half an edit, a fragment-order latent, the pinned wave-per-sequence kernel."""
    lib = _lib.load()
    m, s, fake = _lib.SynModel(), _lib.SynStep(), 256          # non-NULL stand-in pointer
    s.n_clips, s.n_variants = 1, 1
    call = lambda e: lib.syn_denoise_step_edit(ctypes.byref(m), ctypes.byref(s), ctypes.byref(e), None)
    for keep, known in ((fake, None), (None, fake)):
        assert call(_lib.SynEdit(keep, known)) != 0
        msg = lib.syn_last_error()
        assert b"keep" in msg and b"known" in msg and b"NULL" in msg, msg
    s.x_fragment_order = 1
    assert call(_lib.SynEdit(fake, fake)) != 0 and b"x_fragment_order" in lib.syn_last_error()
    s.x_fragment_order, s.reserved = 0, 5
    assert call(_lib.SynEdit(fake, fake)) != 0 and b"reserved = 5" in lib.syn_last_error()
    s.reserved = 8 + 5                                          # (the low three bits select the kernel)
    assert call(_lib.SynEdit(fake, fake)) != 0 and b"reserved = 5" in lib.syn_last_error()


def test_keep_mask_channel_thirds_and_frames():
    m = longform.keep_mask(88)
    assert m.shape == (88, 1536) and m.dtype is torch.bool
    assert m[:, 1024:].all() and not m[:, :1024].any()                                # default: the lower body
    m = longform.keep_mask(88, ("upper", "hands"))
    assert m[:, :1024].all() and not m[:, 1024:].any()
    m = longform.keep_mask(88, ("hands",), frames=(10, 21))
    assert m[:, 512:1024].all() and m[10:21].all()
    assert not m[:10, :512].any() and not m[21:, :512].any() and not m[:10, 1024:].any() and not m[21:, 1024:].any()
    m = longform.keep_mask(32, (), frames=[(0, 11), (20, 32)])                         # "keep frames 0-10 and 20-31, fill the gap"
    assert m[:11].all() and m[20:].all() and not m[11:20].any()
    assert not longform.keep_mask(8, ()).any()
    with pytest.raises(ValueError):
        longform.keep_mask(8, ("legs",))
    with pytest.raises(ValueError):
        longform.keep_mask(8, (), frames=(4, 9))


class _Recorder:
    """A stand-in diffusion: records every window's y and returns a sample that names its window."""
    def __init__(self):
        self.ys = []

    def p_sample_loop(self, model, shape, model_kwargs=None, **kw):
        self.ys.append(model_kwargs["y"])
        return torch.full(shape, float(len(self.ys)))


def test_sample_long_window_slices_line_up_with_window_plan():
    n, B = 128 + 2 * 112, 2
    round_l, rounds, _ = longform.window_plan(n)
    assert (round_l, rounds) == (112, 3)
    g = torch.Generator().manual_seed(3)
    audio, word = torch.zeros(B, n * longform.AUDIO_PER_POSE), torch.zeros(B, n, dtype=torch.long)
    known = torch.arange(n // 4).float().view(1, -1, 1).expand(B, n // 4, 1536).contiguous()      # the value of an entry is its latent frame
    known = known + torch.arange(B).float().view(B, 1, 1) * 1000.0
    keep = longform.keep_mask(n // 4, ("lower",), frames=(10, 21))                                # (n/4, 1536): broadcast over the takes
    rec = _Recorder()
    out = longform.sample_long(rec, None, audio, word, known, n, edit=(known, keep))
    assert out.shape == (B, 3 * 28 + 4, 1536) and len(rec.ys) == 3
    for i, y in enumerate(rec.ys):
        motion, mask = y["inpainted_motion"], y["inpainting_mask"]
        assert motion.shape == mask.shape == (B, 1536, 1, 32) and mask.dtype is torch.bool
        assert motion.is_contiguous() and mask.is_contiguous()
        frames = torch.arange(28 * i, 28 * i + 32).float()                                         # window i: latent frames 28 i .. 28 i + 31
        for b in range(B):
            assert torch.equal(motion[b, :, 0, :], (frames + 1000.0 * b).expand(1536, 32))
        assert torch.equal(mask[0, :, 0, :], keep[28 * i:28 * i + 32].T) and torch.equal(mask[0], mask[1])
    # edit=None: today's y, no in-painting keys
    rec = _Recorder()
    longform.sample_long(rec, None, audio, word, known, n)
    assert all("inpainting_mask" not in y and "inpainted_motion" not in y for y in rec.ys)
    with pytest.raises(ValueError):                             # a take shorter than its last window
        longform.sample_long(_Recorder(), None, audio, word, known, n, edit=(known[:, :80], keep[:80]))
    with pytest.raises(ValueError):
        longform.sample_long(_Recorder(), None, audio, word, known, n, edit=(known, keep.float()))


def test_fusable_takes_the_edit_pair_only(monkeypatch):
    """Both keys and a bool mask: the fused loop.  A mask alone (the reference ignores it) and a float mask stay on the generic path."""
    from syntalker_amd import process
    stub = torch.nn.Linear(1, 1).eval()
    monkeypatch.setattr(process, "resolve", lambda model: (stub, lambda y: None))
    d = process.create_gaussian_diffusion()
    shape = (2, 1536, 1, 32)
    mask, motion = torch.zeros(shape, dtype=torch.bool), torch.zeros(shape)
    fusable = lambda y: d._fusable(stub, {"y": y}, None, None, False, False, False, False, shape)[0] is not None
    assert fusable({})
    assert fusable({"inpainting_mask": mask, "inpainted_motion": motion})
    assert fusable({"inpainted_motion": motion})                           # no mask: no edit, in the reference as here
    assert not fusable({"inpainting_mask": mask})
    assert not fusable({"inpainting_mask": mask.float(), "inpainted_motion": motion})
    assert not fusable({"inpainting_mask": mask[:1], "inpainted_motion": motion})
    assert not fusable({"inpainting_mask": mask, "inpainted_motion": motion[:, :, :, :16]})
    assert d.last_path is None


def test_last_path_names_the_generic_loop():
    from syntalker_amd.process import create_gaussian_diffusion

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor(0.5))

        def forward(self, x, t, y=None):
            return self.w * x
    shape = (1, 1536, 1, 32)
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[:, 1024:] = True
    motion = torch.randn(shape)
    for ddim in (False, True):
        d = create_gaussian_diffusion(use_ddim=ddim)
        loop = d.ddim_sample_loop if ddim else d.p_sample_loop
        out = loop(Toy(), shape, clip_denoised=False, model_kwargs={"y": {"inpainting_mask": mask, "inpainted_motion": motion}},
                   skip_timesteps=d.num_timesteps - 3)
        assert d.last_path == "generic"
        assert torch.equal(out[mask], motion[mask])              # the last step is t = 0: x_next = x0, kept entries are the motion's
        with pytest.raises(AttributeError):
            d.last_path = "fused"


@pytest.mark.parametrize("use_ddim", [False, True])
@pytest.mark.parametrize("steps", [1, 2, 5])
def test_oracle_all_true_mask_returns_the_motion_exactly(use_ddim, steps):
    """At t = 0 both updates reduce to x0 (posterior_mean_coef1[0] = 1, coef2[0] = 0; alphas_cumprod_prev[0] = 1), and x0 is the blend:
    with an all-True mask the loop returns `inpainted_motion` bit for bit, whatever the model says and however many steps ran."""
    from oracle.process_ref import RefProcess
    g = torch.Generator().manual_seed(7 + steps)
    shape = (2, 1536, 1, 32)
    motion = torch.randn(shape, generator=g)
    y = {"inpainting_mask": torch.ones(shape, dtype=torch.bool), "inpainted_motion": motion}
    proc = RefProcess(use_ddim)
    loop = proc.ddim_sample_loop if use_ddim else proc.p_sample_loop
    model_fn = lambda x, t, yy: 0.3 * x + t.float().view(-1, 1, 1, 1) * 1e-3
    out = loop(model_fn, shape, y, noise=torch.randn(shape, generator=g), step_noise=torch.randn(steps, *shape, generator=g),
               skip_timesteps=proc.num_timesteps - steps)
    assert torch.equal(out, motion)
