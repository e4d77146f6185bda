"""Torch restatement of the T2M evaluator (utils/t2m_eval_tools.py:332-351, 564-639, 866-899) over its state dicts, fp32 on the CPU: the
checker of tests/test_gpu_t2m_evaluator.py and of smoke().  nn.GRU with pack_padded_sequence is used here because this is the comparison,
not a product path."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence


def movement(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """(N, T, 619) -> (N, T'', 512)."""
    h = F.leaky_relu(F.conv1d(x.transpose(1, 2), sd["main.0.weight"], sd["main.0.bias"], stride=2, padding=1), 0.2)
    h = F.leaky_relu(F.conv1d(h, sd["main.3.weight"], sd["main.3.bias"], stride=2, padding=1), 0.2)
    return F.linear(h.transpose(1, 2), sd["out_net.weight"], sd["out_net.bias"])


def make_gru(sd: dict) -> torch.nn.GRU:
    h = sd["hidden"].shape[-1]
    gru = torch.nn.GRU(h, h, batch_first=True, bidirectional=True).to(sd["hidden"].device)
    gru.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("gru.")})
    return gru


def bigru_head(sd: dict, x: torch.Tensor, lens, gru=None) -> torch.Tensor:
    """input already embedded (N, L, H); lens in any order -> output_net(forward final | reverse final), row i = sequence i.
    `gru`: make_gru(sd) built once by a caller that times this."""
    h = sd["hidden"].shape[-1]
    gru = gru or make_gru(sd)
    packed = pack_padded_sequence(x, torch.as_tensor(lens).tolist(), batch_first=True, enforce_sorted=False)
    _, last = gru(packed, sd["hidden"].repeat(1, x.shape[0], 1))
    y = F.linear(torch.cat([last[0], last[1]], dim=-1), sd["output_net.0.weight"], sd["output_net.0.bias"])
    y = F.leaky_relu(F.layer_norm(y, (h,), sd["output_net.1.weight"], sd["output_net.1.bias"]), 0.2)
    return F.linear(y, sd["output_net.3.weight"], sd["output_net.3.bias"])


@torch.no_grad()
def motion_embeddings(state: dict, motions: torch.Tensor, m_lens, aligned: bool = True, gru=None) -> torch.Tensor:
    """get_motion_embeddings: rows in align_idx order (longest first) unless aligned=False (row i = motion i)."""
    m_lens = torch.as_tensor(m_lens)
    idx = align_idx(m_lens) if aligned else np.arange(len(m_lens))
    sd = state["motion_encoder"]
    mv = movement(state["movement_encoder"], motions.float()[idx][..., :-4])
    return bigru_head(sd, F.linear(mv, sd["input_emb.weight"], sd["input_emb.bias"]), m_lens[idx] // 4, gru)


@torch.no_grad()
def text_embeddings(state: dict, word_embs, pos_onehot, cap_lens, gru=None) -> torch.Tensor:
    sd = state["text_encoder"]
    x = word_embs.float() + F.linear(pos_onehot.float(), sd["pos_emb.weight"], sd["pos_emb.bias"])
    return bigru_head(sd, F.linear(x, sd["input_emb.weight"], sd["input_emb.bias"]), cap_lens, gru)


def co_embeddings(state: dict, word_embs, pos_onehot, cap_lens, motions, m_lens):
    """get_co_embeddings: (text, motion), both in align_idx order."""
    idx = align_idx(torch.as_tensor(m_lens))
    return text_embeddings(state, word_embs, pos_onehot, cap_lens)[idx], motion_embeddings(state, motions, m_lens)


def align_idx(m_lens) -> np.ndarray:
    return np.argsort(torch.as_tensor(m_lens).tolist())[::-1].copy()


def build_state(shift: int = 0) -> dict:
    """The evaluator's three state dicts with synth's seeded weights (shift 0: the fixture's)."""
    from syntalker_amd import synth, t2m_evaluator as te
    mods = {"movement_encoder": te.MovementConvEncoder(619, 512, 512), "text_encoder": te.TextEncoderBiGRUCo(300, 15, 512, 512),
            "motion_encoder": te.MotionEncoderBiGRUCo(512, 1024, 512)}
    return {k: synth.synth_t2m_state_dict(m, synth.T2M_STATE_SEEDS[k] + shift) for k, m in mods.items()}
