"""Deterministic synthetic weights and inputs for the denoising hot path.

There is no network for checkpoints or datasets, so benchmarks, parity tests and the
golden-vector generator all draw weights and inputs from the same name-keyed, seed-keyed
CPU generators.  Everything here is plain CPU torch so the same bytes are produced in the
build container (where the reference is importable) and on the GPU box (where it is not).

Shapes follow the reference call sites:
  x_T / noise   (B, 1536, 1, 32)   diffusion_rvqvae_trainer.py:444
  audio         (B, 68224, 2)      diffusion_rvqvae_trainer.py:422  (16000//30 * 128 samples)
  word          (B, 128) int64     diffusion_rvqvae_trainer.py:433-442
  seed          (B, 4, 1536)       diffusion_rvqvae_trainer.py:428-431
  style_feature (B, 512) zeros for denoiser.MDM (:442) / (B, 256) for denoiser_h3d.MDM
  mask          (B, 1, 1, 32) bool diffusion_rvqvae_trainer.py:347
"""
from __future__ import annotations

import zlib
from types import SimpleNamespace

import torch

LATENT_C = 1536      # 3 body parts x 512 RVQ latent channels
LATENT_T = 32        # 128 pose frames / vqvae_squeeze_scale 4
AUDIO_LEN = 16000 // 30 * 128   # 68224, test-path length
VOCAB = 11195
WORD_DIM = 300


def default_args(**over):
    """The argparse keys MDM.__init__ reads (models/denoiser.py:36-71), yaml defaults of
    configs/diffusion_rvqvae_128.yaml."""
    a = dict(vqvae_type="rvqvae", use_motionclip=False, audio_rep="onset+amplitude",
             audio_f=256, word_f=256, data_path="", t_fix_pre=False, vqvae_squeeze_scale=4)
    a.update(over)
    return SimpleNamespace(**a)


def _gen(name: str, seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
    return g


def synth_tensor(name: str, shape, seed: int = 0) -> torch.Tensor | None:
    """Value for one state_dict entry, or None to leave the module's own value (deterministic
    buffers: positional table, rotary inv_freq, BatchNorm counters)."""
    shape = tuple(shape)
    leaf = name.rsplit(".", 1)[-1]
    if leaf in ("pe", "inv_freq", "num_batches_tracked"):
        return None
    g = _gen(name, seed)
    if leaf == "running_var":
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == "running_mean":
        return 0.1 * torch.randn(shape, generator=g)
    if leaf == "codebook":              # residual VQ: layer q quantises what layers < q left over (models/vq/residual_vq.py)
        q = int(name.split(".")[-2])
        return 0.06 * (0.6 ** q) * torch.randn(shape, generator=g)
    if name.startswith("uncon_"):
        return 0.5 * torch.randn(shape, generator=g)
    if name == "text_pre_encoder_body.weight":
        return 0.3 * torch.randn(shape, generator=g)
    if len(shape) == 1:
        is_norm_scale = leaf == "weight"
        if is_norm_scale:               # LayerNorm / BatchNorm gamma
            return 1.0 + 0.1 * torch.randn(shape, generator=g)
        return 0.05 * torch.randn(shape, generator=g)   # every bias / beta
    fan_in = 1
    for s in shape[1:]:
        fan_in *= s
    return torch.randn(shape, generator=g) * (fan_in ** -0.5)


@torch.no_grad()
def synth_fill_(module_or_sd, seed: int = 0):
    """Overwrite every entry of a state_dict (or a module's) in place with synth_tensor()."""
    sd = module_or_sd if isinstance(module_or_sd, dict) else module_or_sd.state_dict()
    for k, v in sd.items():
        t = synth_tensor(k, v.shape, seed)
        if t is not None:
            v.copy_(t.to(v.dtype))
    return module_or_sd


def synth_clip_inputs(batch: int, seed: int = 0, style_dim: int = 512, style_zero: bool = True,
                      mask_batch: int | None = None):
    """model_kwargs['y'] exactly as the trainers build it, on CPU."""
    g = _gen("inputs", seed)
    y = {
        "audio": torch.randn(batch, AUDIO_LEN, 2, generator=g),
        "word": torch.randint(0, VOCAB, (batch, 128), generator=g),
        "id": torch.zeros(batch, 1, dtype=torch.long),
        "seed": torch.randn(batch, 4, LATENT_C, generator=g),
        "mask": torch.ones(mask_batch or batch, 1, 1, LATENT_T, dtype=torch.bool),
    }
    if style_zero:
        y["style_feature"] = torch.zeros(batch, style_dim)
    else:
        y["style_feature"] = torch.randn(batch, style_dim, generator=g)
    return y


def synth_latent(batch: int, seed: int = 0, name: str = "x_T") -> torch.Tensor:
    return torch.randn(batch, LATENT_C, 1, LATENT_T, generator=_gen(name, seed))


def synth_step_noise(steps: int, batch: int, seed: int = 0) -> torch.Tensor:
    """Pre-drawn per-step noise (K, B, 1536, 1, 32); row k is used by the k-th executed step."""
    return torch.randn(steps, batch, LATENT_C, 1, LATENT_T, generator=_gen("step_noise", seed))


def to_device(y: dict, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in y.items()}


# ---- RVQ-VAE (the models either side of the sampling loop): synthetic weights / poses / latents ----------------------
def synth_vq_state_dict(dim: int, seed: int = 11) -> dict:
    from . import rvqvae
    sd = {k: torch.zeros_like(v) for k, v in rvqvae.build(dim).state_dict().items()}
    return synth_fill_(sd, seed)


def synth_vq_pose(part: str, dim: int, n: int = 2, t: int = 64, seed: int = 3) -> torch.Tensor:
    return synth_tensor(f"vq.pose.{part}", (n, t, dim), seed=seed) * dim ** 0.5           # N(0,1) entries


def synth_vq_rec_latent(sd: dict, part: str, n: int = 2, t: int = 16) -> torch.Tensor:
    """A latent the residual quantiser has something to say about: a sum of one code per layer (indices from a seeded
    generator) plus noise at 30 % of the last layer's scale -- what the sampler's output looks like after training."""
    from .rvqvae import NB_CODE, NUM_Q
    g = _gen(f"vq.rec.idx.{part}", 4)
    rec = 0.3 * 0.06 * 0.6 ** 5 * synth_tensor(f"vq.rec.{part}", (n, t, 512), seed=4) * (n * t * 512) ** 0.5
    for q in range(NUM_Q):
        idx = torch.randint(0, NB_CODE, (n, t), generator=g)
        rec = rec + sd[f"quantizer.layers.{q}.codebook"].cpu()[idx]
    return rec


def synth_vq_motion(n: int, t: int, dim: int, step: int = 0, seed: int = 61) -> torch.Tensor:
    """A batch (n, t, dim) of structured motion for codec-training runs: per channel a sum of three sinusoids whose frequencies and
    amplitudes belong to the "dataset" (`seed`), per clip a start time and a gain drawn for batch number `step`."""
    g = _gen("vq.motion.dataset", seed)
    freq = 0.02 + 0.2 * torch.rand(3, dim, generator=g)                       # cycles per frame
    amp = torch.rand(3, dim, generator=g) * torch.tensor([1.0, 0.5, 0.25]).view(3, 1)
    phase = 6.283185307179586 * torch.rand(3, dim, generator=g)
    gb = _gen(f"vq.motion.batch.{step}", seed)
    t0 = 1000.0 * torch.rand(n, 1, 1, 1, generator=gb)
    gain = 0.75 + 0.5 * torch.rand(n, 1, 1, generator=gb)
    frames = torch.arange(t, dtype=torch.float32).view(1, t, 1, 1) + t0
    return gain * (amp * torch.sin(6.283185307179586 * freq * frames + phase)).sum(dim=2)


# ---- a long take for the chunked driver (diffusion_rvqvae_trainer.py:359-541): what `_load_data` hands `_g_test` ---------------
def synth_long_take(n_pose: int, seed: int = 21) -> dict:
    """One take (batch 1, as the reference's test loader delivers it): axis-angle pose (1, n, 165), audio (1, n*533, 2),
    word ids (1, n), ground-truth latents (1, n/4, 1536) (only their first `pre_frames` rows are ever read)."""
    g = _gen("long_take", seed)
    return {"pose": 0.3 * torch.randn(1, n_pose, 165, generator=g),
            "audio": torch.randn(1, n_pose * (16000 // 30), 2, generator=g),
            "word": torch.randint(0, VOCAB, (1, n_pose), generator=g),
            "latent": torch.randn(1, n_pose // 4, LATENT_C, generator=g)}


def synth_long_noise(window: int, steps: int, seed: int = 22):
    """(x_T (1,1536,1,32), per-step noise (steps,1,1536,1,32)) of window `window` of a long take."""
    g = _gen(f"long_noise.{window}", seed)
    return torch.randn(1, LATENT_C, 1, LATENT_T, generator=g), torch.randn(steps, 1, LATENT_C, 1, LATENT_T, generator=g)


def synth_joint_masks() -> dict:
    """0/1 masks over the 165 axis-angle channels with the reference's counts per body part (13 / 30 / 9 joints,
    diffusion_rvqvae_trainer.py:52-60); which joints they are does not matter to the path under test."""
    import numpy as np
    m = {k: np.zeros(165) for k in ("upper", "hands", "lower")}
    for j in (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21):
        m["upper"][3 * j:3 * j + 3] = 1
    m["hands"][75:165] = 1
    for j in (0, 1, 2, 4, 5, 7, 8, 10, 11):
        m["lower"][3 * j:3 * j + 3] = 1
    return m


def synth_pose_stats(seed: int = 23) -> dict:
    """(mean, std) per body part and for the root velocity: seeded stand-ins for mean_std/*.npy (trainer :187-224)."""
    g = _gen("pose_stats", seed)
    out = {}
    for name, dim in (("upper", 78), ("hands", 180), ("lower", 54), ("trans", 3)):
        out[name] = (0.2 * torch.randn(dim, generator=g), 0.5 + torch.rand(dim, generator=g))
    return out


# ---- the text-prompt (h3d) trainer's test scenario (h3d_diffusion_new_trainer.py:465-615) ---------------------------------------
H3D_PROMPTS = {"upper": "a person waves the right hand", "lower": "a person walks forward"}


def synth_prompt_vector(prompt: str) -> torch.Tensor:
    """(1, 256) stand-in for `textencoder(prompt).loc` (the TMR text encoder's mean, :489-511), seeded by the prompt's text."""
    return torch.randn(1, 256, generator=_gen("prompt:" + prompt, 25))


def synth_h3d_part_index() -> dict:
    """Disjoint index sets over the 623 HumanML3D-style pose channels with the reference's counts per body part (156 / 360 / 107)."""
    perm = torch.randperm(623, generator=_gen("h3d_parts", 26))
    return {"upper": perm[:156].sort().values, "hands": perm[156:516].sort().values, "lower": perm[516:].sort().values}


def synth_pose_clip(batch: int, n_pose: int, seed: int = 27) -> dict:
    """What the dataloader hands `_load_data` (diffusion_rvqvae_trainer.py:245-249): axis-angle poses (B, n, 165) - rotations up to ~1.5 rad,
    a few exactly zero (the small-angle branch of the conversion) - and the root velocity (B, n, 3)."""
    g = _gen("pose_clip", seed)
    pose = 0.5 * torch.randn(batch, n_pose, 165, generator=g)
    pose[:, ::7, 9:12] = 0.0
    return {"pose": pose, "trans_v": 0.05 * torch.randn(batch, n_pose, 3, generator=g)}


# ---- TMR encoders (h3d_diffusion_new_trainer.py:168-176): weights, motion features, an offline DistilBERT ------------------------------
TMR_NFEATS = 623
TMR_PROMPTS = ["a person waves the right hand", "someone walks forward slowly and then turns around to look back",
               "a man jumps"]
TMR_PROMPT_ONE = "a person raises both arms above the head"
_TMR_WORDS = ("a person waves the right left hand someone walks forward slowly and then turns around to look back man jumps raises both "
              "arms above head walk run sit stand up down kick dance").split()


def synth_tmr_state_dict(module: torch.nn.Module, seed: int = 31) -> dict:
    """The seeded weights of a TMR encoder with the reference's keys (every entry but the positional table: LayerNorm gamma = 1 + 0.1 N(0,1),
    beta / biases / distribution tokens 0.05 N(0,1), matrices N(0, 1/fan_in)); `module` supplies the keys and shapes."""
    sd = {k: torch.zeros_like(v) for k, v in module.state_dict().items()}
    for k, v in module.state_dict().items():
        if synth_tensor(k, v.shape, seed) is None:
            sd[k] = v.detach().clone()
    return synth_fill_(sd, seed)


def synth_tmr_motion(batch: int, frames: int = 128, seed: int = 32) -> torch.Tensor:
    """(B, frames, 623) stand-in for the h3d loader's `tmr_tar_pose` (normalised HumanML3D features: unit scale)."""
    return torch.randn(batch, frames, TMR_NFEATS, generator=_gen("tmr_motion", seed))


def synth_tmr_text_model(path: str, seed: int = 33, layers: int = 2):
    """Write an offline DistilBERT directory (synthetic vocab.txt, 768-wide config of `layers` layers, seeded weights, tokenizer files) that
    `AutoTokenizer / AutoModel.from_pretrained(path)` read without a network."""
    import os
    from transformers import DistilBertConfig, DistilBertModel, DistilBertTokenizer
    os.makedirs(path, exist_ok=True)
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + sorted(set(_TMR_WORDS))
    with open(os.path.join(path, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    cfg = DistilBertConfig(vocab_size=len(vocab), dim=768, n_layers=layers, n_heads=12, hidden_dim=3072, max_position_embeddings=512)
    model = DistilBertModel(cfg)
    synth_fill_(model, seed)
    model.save_pretrained(path)
    DistilBertTokenizer(os.path.join(path, "vocab.txt"), do_lower_case=True).save_pretrained(path)
    return path


TMR_RAGGED_TOKENS = (2, 16, 17, 64, 65, 254)      # token counts each side of a 16-row MFMA tile and of a 64-query tile, the empty prompt, the maximum


def synth_tmr_prompts(token_lengths, seed: int = 35) -> list:
    """Prompts of exactly `token_lengths` tokens each ([CLS] + words + [SEP]; every word of the synthetic vocabulary is one token, 2 tokens is
    the empty prompt), the words a seeded draw from the synthetic word list."""
    words = sorted(set(_TMR_WORDS))
    g = _gen("tmr_prompts", seed)
    out = []
    for n in token_lengths:
        if n < 2:
            raise ValueError("a tokenized prompt has at least [CLS] and [SEP]")
        out.append(" ".join(words[i] for i in torch.randint(0, len(words), (n - 2,), generator=g).tolist()))
    return out


def synth_evaluator_state_dict(module: torch.nn.Module, seed: int = 41) -> dict:
    """The seeded weights of a VAESKConv with the reference's keys: matrices N(0, 1/fan_in) over the WHOLE conv weight (values outside the
    masks too, which only the masks keep out of the result), GroupNorm gains 1 + 0.1 N(0,1), biases 0.05 N(0,1); the neighbour masks and the
    pooling matrices (`common.0.weight`) stay as the module builds them."""
    sd = {}
    for k, v in module.state_dict().items():
        keep = k.endswith(".mask") or k.endswith("common.0.weight")
        sd[k] = v.detach().clone() if keep else synth_tensor(k, v.shape, seed).to(v.dtype)
    return sd


def synth_evaluator_takes(lengths, seed: int, scale: float = 1.0, shift: float = 0.0) -> list:
    """Takes of (n, 330) 6D-pose stand-ins (unit Gaussian, scaled and shifted), one per length."""
    g = _gen("evaluator_takes", seed)
    return [scale * torch.randn(n, 330, generator=g) + shift for n in lengths]


def synth_evaluator_input(batch: int, frames: int, seed: int = 42) -> torch.Tensor:
    """(B, frames, 330) input of the evaluator's golden cases."""
    return torch.randn(batch, frames, 330, generator=_gen("evaluator_input", seed))


EVALUATOR_CASES = ((2, 256, 42), (1, 1024, 43), (3, 16, 44))            # (B, n, seed) of tests/golden/evaluator_outputs.npz
EVALUATOR_FGD_TAKES = {"tar": ((2000, 3300, 1500, 2600, 1000), 45, 1.0, 0.0), "rec": ((1800, 2900, 3100, 1333, 2400), 46, 0.9, 0.05)}


def synth_smplx_model(data_path_1: str, parents) -> str:
    """Write the one part of the SMPL-X model file the FGD evaluator reads - `kintree_table` - where VAESKConv looks for it under
    `data_path_1`; returns the file's path."""
    import os
    import numpy as np
    path = os.path.join(data_path_1, "smplx_models", "smplx", "SMPLX_NEUTRAL_2020.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, kintree_table=np.stack([np.asarray(parents, np.int64), np.arange(len(parents))]))
    return path


# ---- T2M text-motion evaluator (utils/t2m_eval_tools.py): weights of its three modules and loader-shaped batches ---------------------------
T2M_FRAMES, T2M_TEXT_LEN, T2M_DIM_POSE = 196, 22, 623            # the h3d loader's padded shapes (max_motion_length, max_text_len + 2)
T2M_STATE_SEEDS = {"movement_encoder": 51, "text_encoder": 52, "motion_encoder": 53}     # finest.tar's three dicts, tests/golden/t2m_evaluator_outputs.npz


def synth_t2m_state_dict(module: torch.nn.Module, seed: int = 51) -> dict:
    """Seeded weights of a MovementConvEncoder / MotionEncoderBiGRUCo / TextEncoderBiGRUCo at the scale the reference initialises them:
    Xavier-normal Linear and Conv1d weights (its `init_weight`), GRU weights and biases uniform in +-1/sqrt(H) (torch's default), the other
    biases 0.05 N(0,1) instead of its zeros, LayerNorm gains 1 + 0.1 N(0,1), `hidden` N(0,1); `module` supplies the keys and shapes."""
    sd = {}
    for k, v in module.state_dict().items():
        g = _gen("t2m:" + k, seed)
        shape = tuple(v.shape)
        if k == "hidden":
            t = torch.randn(shape, generator=g)
        elif k.startswith("gru."):
            bound = shape[-1] ** -0.5 if len(shape) == 2 else (shape[0] // 3) ** -0.5
            t = (2 * torch.rand(shape, generator=g) - 1) * bound
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g) if k.endswith("output_net.1.weight") else 0.05 * torch.randn(shape, generator=g)
        else:
            field = 1
            for s in shape[2:]:
                field *= s
            t = torch.randn(shape, generator=g) * (2.0 / ((shape[0] + shape[1]) * field)) ** 0.5
        sd[k] = t.to(v.dtype)
    return sd


def synth_t2m_batch(n: int, seed: int, frames: int = T2M_FRAMES, text_len: int = T2M_TEXT_LEN, m_range=(40, T2M_FRAMES), cap_range=(4, T2M_TEXT_LEN),
                    m_lens=None, cap_lens=None) -> tuple:
    """One batch as the h3d evaluation loader collates it: (word_embs (n, text_len, 300), pos_onehot (n, text_len, 15), cap_lens (n) int64
    descending, motions (n, frames, 623) zero beyond each motion's frames, m_lens (n) int64).  Lengths are drawn from the closed ranges unless
    given; token slots beyond a caption hold values (the loader's padding tokens), which a packed sequence never reads."""
    g = _gen("t2m_batch", seed)
    if m_lens is None:
        m_lens = torch.randint(m_range[0], min(m_range[1], frames) + 1, (n,), generator=g)
    if cap_lens is None:
        cap_lens = torch.randint(cap_range[0], min(cap_range[1], text_len) + 1, (n,), generator=g).sort(descending=True).values
    m_lens, cap_lens = torch.as_tensor(m_lens, dtype=torch.int64), torch.as_tensor(cap_lens, dtype=torch.int64)
    word = 0.4 * torch.randn(n, text_len, WORD_DIM, generator=g)
    pos = torch.nn.functional.one_hot(torch.randint(0, 15, (n, text_len), generator=g), 15).float()
    motions = torch.randn(n, frames, T2M_DIM_POSE, generator=g)
    motions = motions * (torch.arange(frames)[None, :, None] < m_lens[:, None, None])
    return word, pos, cap_lens, motions, m_lens
