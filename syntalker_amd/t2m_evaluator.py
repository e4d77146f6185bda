"""The reference's T2M text-motion co-embedding evaluator (utils/t2m_eval_tools.py) on the HIP kernels (include/syn_hip.h:
syn_t2m_encode_motion / syn_t2m_encode_text).

The h3d trainer's `eval()` (h3d_diffusion_new_trainer.py:906-1059) scores every replication with `EvaluatorMDMWrapper` (:833-899): the
movement encoder (two stride-2 convolutions and a Linear, :332-351) and a bidirectional GRU over its output (`MotionEncoderBiGRUCo`,
:606-639) embed a motion; a bidirectional GRU over word vectors (`TextEncoderBiGRUCo`, :564-603) embeds its caption; Matching Score,
R-precision, FID, Diversity and MultiModality are read off those 512-vectors (syntalker_amd.metrics).

The three modules keep the reference's constructor arguments and state_dict keys, so `finest.tar`'s three dicts load strictly.  Eval-only,
fp32, dropout the identity.  `nn.GRU` on ROCm is MIOpen, which DESIGN.md rules out of a product path: the modules here hold parameters and
never run torch arithmetic; a module or input on the CPU raises SynHipError (no fallback).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
from torch import nn

from . import _lib, engine

UNIT_LENGTH = 4                  # frames per movement-encoder step (two stride-2 convolutions)
POS_SIZE = _lib.SYN_T2M_POS      # len(POS_enumerator) (utils/t2m_eval_tools.py: the 15 part-of-speech tags)
CHUNK = 4096                     # sequences per library call: bounds the workspace (W_ih x of every step: 1.2 MB per motion of 196 frames)


def conv_len(t: int) -> int:
    """Output frames of Conv1d(kernel 4, stride 2, padding 1)."""
    return (t - 2) // 2 + 1


class _EvalOnly(nn.Module):
    __getstate__ = engine.drop_caches         # (deepcopy / torch.save: without the packed copy)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} is part of the T2M evaluator, an inference module here (the reference's "
                                      "wrapper calls .eval() on it, utils/t2m_eval_tools.py:861-863); training it is not built")
        return super().train(False)

    def _device(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.SynHipError(f"{type(self).__name__} runs on the HIP kernels only: move the module to the GPU (no CPU fallback)")
        return dev

    def _cached(self, build):
        def fill(p):
            p["idx"] = {}
            build(p, self._device())
        return engine.derived(self, list(self.parameters()), fill)


def _pack(p: dict, w: torch.Tensor, conv_cin: int = 0, layout: int = 0) -> int:
    """syn_t2m_pack_weight of one weight; the packed tensor is kept alive in p['keep'], its pointer returned."""
    w = w.detach().float().contiguous()
    n = w.shape[0]
    k = w[0].numel()
    floats = 3 * layout * layout if layout else -(-n // 128) * 128 * (-(-k // 16) * 16)
    out = torch.empty(floats, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().syn_t2m_pack_weight(w.data_ptr(), n, k, conv_cin, layout, out.data_ptr(), _lib.current_stream(w.device)),
               "syn_t2m_pack_weight")
    p["keep"] += [w, out]
    return out.data_ptr()


def _plain(p: dict, t: torch.Tensor) -> int:
    t = t.detach().float().contiguous()
    p["keep"].append(t)
    return t.data_ptr()


def _pack_gru(p: dict, gru: nn.GRU, hidden: torch.Tensor, h: int) -> _lib.SynT2mGru:
    if gru.hidden_size != h or gru.input_size != h or gru.num_layers != 1 or not gru.bidirectional:
        raise NotImplementedError(f"the HIP recurrent kernel is built for a one-layer bidirectional GRU({h}, {h}), got "
                                  f"GRU({gru.input_size}, {gru.hidden_size}, layers {gru.num_layers})")
    g = _lib.SynT2mGru()
    g.w_ih = _pack(p, torch.cat([gru.weight_ih_l0, gru.weight_ih_l0_reverse]))
    g.b_ih = _plain(p, torch.cat([gru.bias_ih_l0, gru.bias_ih_l0_reverse]))
    g.w_hh[0] = _pack(p, gru.weight_hh_l0, layout=h)
    g.w_hh[1] = _pack(p, gru.weight_hh_l0_reverse, layout=h)
    g.b_hh = _plain(p, torch.cat([gru.bias_hh_l0, gru.bias_hh_l0_reverse]))
    g.hidden = _plain(p, hidden.reshape(2, h))
    return g


def _pack_head(p: dict, net: nn.Sequential, h: int) -> _lib.SynT2mHead:
    if net[0].weight.shape != (h, 2 * h) or net[3].weight.shape != (_lib.SYN_T2M_EMB, h):
        raise NotImplementedError(f"the HIP evaluator is built for output_net {2 * h} -> {h} -> {_lib.SYN_T2M_EMB}")
    return _lib.SynT2mHead(_pack(p, net[0].weight), _plain(p, net[0].bias), _plain(p, net[1].weight), _plain(p, net[1].bias),
                           _pack(p, net[3].weight), _plain(p, net[3].bias))


def _output_net(hidden_size: int, output_size: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(hidden_size * 2, hidden_size), nn.LayerNorm(hidden_size), nn.LeakyReLU(0.2, inplace=True),
                         nn.Linear(hidden_size, output_size))


def _lengths(p: dict, kind: int, lens: np.ndarray, dev):
    """Device copies of one call's lengths and, per chunk of CHUNK sequences, the tile order (longest first).  Cached by value, so a call
    repeated with the same lengths - a graph capture after its warm call - uploads nothing."""
    key = (kind, lens.tobytes())
    hit = p["idx"].get(key)
    if hit is None:
        if len(p["idx"]) > 7:
            p["idx"].clear()
        order = [np.argsort(-lens[i:i + CHUNK], kind="stable").astype(np.int32) for i in range(0, len(lens), CHUNK)]
        hit = (torch.from_numpy(lens.astype(np.int32)).to(dev), [torch.from_numpy(o).to(dev) for o in order])
        p["idx"][key] = hit
    return hit


def _workspace(p: dict, kind: int, n: int, length: int, dev) -> torch.Tensor:
    def nbytes():
        size = int(_lib.load().syn_t2m_workspace_bytes(n, length, kind))
        if size < 0:
            raise ValueError(f"T2M evaluator: {n} sequences of {length} outside what the library takes "
                             f"(at most {_lib.SYN_T2M_MAX_FRAMES} frames / tokens)")
        return size
    return engine.workspace(p["ws"], (kind, n, length), nbytes, dev)


class MovementConvEncoder(_EvalOnly):
    """utils/t2m_eval_tools.py:332-351.  Runs fused with MotionEncoderBiGRUCo (`embed_motions`)."""

    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.main = nn.Sequential(nn.Conv1d(input_size, hidden_size, 4, 2, 1), nn.Dropout(0.2, inplace=True), nn.LeakyReLU(0.2, inplace=True),
                                  nn.Conv1d(hidden_size, output_size, 4, 2, 1), nn.Dropout(0.2, inplace=True), nn.LeakyReLU(0.2, inplace=True))
        self.out_net = nn.Linear(output_size, output_size)
        super().train(False)

    def packed(self):
        def build(p, dev):
            c1, c2 = self.main[0], self.main[3]
            want = [(_lib.SYN_T2M_MOVE, _lib.SYN_T2M_POSE, 4), (_lib.SYN_T2M_MOVE, _lib.SYN_T2M_MOVE, 4), (_lib.SYN_T2M_MOVE, _lib.SYN_T2M_MOVE)]
            if [tuple(c1.weight.shape), tuple(c2.weight.shape), tuple(self.out_net.weight.shape)] != want:
                raise NotImplementedError("the HIP evaluator is built for MovementConvEncoder(619, 512, 512) (HumanML3D, dim_pose 623)")
            p["ptr"] = (_pack(p, c1.weight, conv_cin=_lib.SYN_T2M_POSE), _plain(p, c1.bias), _pack(p, c2.weight, conv_cin=_lib.SYN_T2M_MOVE),
                        _plain(p, c2.bias), _pack(p, self.out_net.weight), _plain(p, self.out_net.bias))
        return self._cached(build)

    def forward(self, inputs):
        raise NotImplementedError("MovementConvEncoder runs fused with MotionEncoderBiGRUCo: t2m_evaluator.embed_motions / "
                                  "EvaluatorMDMWrapper.get_motion_embeddings")


class MotionEncoderBiGRUCo(_EvalOnly):
    """utils/t2m_eval_tools.py:606-639."""

    def __init__(self, input_size, hidden_size, output_size, device=None):
        super().__init__()
        self.device = device
        self.input_emb = nn.Linear(input_size, hidden_size)
        self.gru = nn.GRU(hidden_size, hidden_size, batch_first=True, bidirectional=True)
        self.output_net = _output_net(hidden_size, output_size)
        self.hidden_size = hidden_size
        self.hidden = nn.Parameter(torch.randn((2, 1, self.hidden_size)))
        super().train(False)

    def packed(self):
        def build(p, dev):
            h = _lib.SYN_T2M_MOTION_H
            if tuple(self.input_emb.weight.shape) != (h, _lib.SYN_T2M_MOVE):
                raise NotImplementedError("the HIP evaluator is built for MotionEncoderBiGRUCo(512, 1024, 512)")
            p["ptr"] = (_pack(p, self.input_emb.weight), _plain(p, self.input_emb.bias))
            p["gru"], p["head"] = _pack_gru(p, self.gru, self.hidden, h), _pack_head(p, self.output_net, h)
        return self._cached(build)

    def forward(self, inputs, m_lens):
        raise NotImplementedError("MotionEncoderBiGRUCo runs fused with MovementConvEncoder: t2m_evaluator.embed_motions / "
                                  "EvaluatorMDMWrapper.get_motion_embeddings")


class TextEncoderBiGRUCo(_EvalOnly):
    """utils/t2m_eval_tools.py:564-603."""

    def __init__(self, word_size, pos_size, hidden_size, output_size, device=None):
        super().__init__()
        self.device = device
        self.pos_emb = nn.Linear(pos_size, word_size)
        self.input_emb = nn.Linear(word_size, hidden_size)
        self.gru = nn.GRU(hidden_size, hidden_size, batch_first=True, bidirectional=True)
        self.output_net = _output_net(hidden_size, output_size)
        self.hidden_size = hidden_size
        self.hidden = nn.Parameter(torch.randn((2, 1, self.hidden_size)))
        super().train(False)

    def packed(self):
        def build(p, dev):
            h = _lib.SYN_T2M_TEXT_H
            if tuple(self.pos_emb.weight.shape) != (_lib.SYN_T2M_WORD, POS_SIZE) or tuple(self.input_emb.weight.shape) != (h, _lib.SYN_T2M_WORD):
                raise NotImplementedError("the HIP evaluator is built for TextEncoderBiGRUCo(300, 15, 512, 512)")
            m = _lib.SynT2mModel()
            m.pos_w, m.pos_b = _pack(p, self.pos_emb.weight), _plain(p, self.pos_emb.bias)
            m.text_in_w, m.text_in_b = _pack(p, self.input_emb.weight), _plain(p, self.input_emb.bias)
            m.text_gru, m.text_head = _pack_gru(p, self.gru, self.hidden, h), _pack_head(p, self.output_net, h)
            p["model"] = m
        return self._cached(build)

    def forward(self, word_embs, pos_onehot, cap_lens):
        """word_embs (N, L, 300), pos_onehot (N, L, 15) fp32 on the GPU, cap_lens N token counts in 1 .. L (any order; the reference needs
        them descending) -> (N, 512), row i = caption i."""
        if not (torch.is_tensor(word_embs) and torch.is_tensor(pos_onehot) and word_embs.is_cuda and pos_onehot.is_cuda):
            raise _lib.SynHipError("TextEncoderBiGRUCo: inputs must be GPU tensors; the evaluator runs on the HIP kernels only (no CPU fallback)")
        p = self.packed()
        if word_embs.dim() != 3 or word_embs.shape[2] != _lib.SYN_T2M_WORD or pos_onehot.shape != (*word_embs.shape[:2], POS_SIZE):
            raise ValueError(f"TextEncoderBiGRUCo: expected word_embs (N, L, {_lib.SYN_T2M_WORD}) and pos_onehot (N, L, {POS_SIZE}), got "
                             f"{tuple(word_embs.shape)} and {tuple(pos_onehot.shape)}")
        n, length = word_embs.shape[:2]
        lens = np.asarray(torch.as_tensor(cap_lens).tolist(), dtype=np.int64).reshape(-1)
        if n < 1 or length < 1 or len(lens) != n or lens.min() < 1 or lens.max() > length:
            raise ValueError(f"TextEncoderBiGRUCo: {n} captions of {length} tokens need N >= 1 lengths in 1 .. {length} "
                             "(pack_padded_sequence refuses the others)")
        dev = word_embs.device
        w, o = word_embs.detach().float().contiguous(), pos_onehot.detach().float().contiguous()
        lens_dev, orders = _lengths(p, _lib.SYN_T2M_TEXT, lens, dev)
        out = torch.empty(n, _lib.SYN_T2M_EMB, device=dev)
        lib, st = _lib.load(), _lib.current_stream(dev)
        for c, order in enumerate(orders):
            i, m = c * CHUNK, len(order)
            _lib.check(lib.syn_t2m_encode_text(C.byref(p["model"]), w[i:i + m].data_ptr(), o[i:i + m].data_ptr(), m, length,
                                               lens_dev[i:i + m].data_ptr(), order.data_ptr(),
                                               _workspace(p, _lib.SYN_T2M_TEXT, m, length, dev).data_ptr(), out[i:i + m].data_ptr(), st),
                       "syn_t2m_encode_text")
        return out


def embed_motions(movement_encoder: MovementConvEncoder, motion_encoder: MotionEncoderBiGRUCo, motions, m_lens) -> torch.Tensor:
    """`motion_encoder(movement_encoder(motions[..., :-4]), m_lens // 4)` in one library call: motions (N, T, 623) fp32 on the GPU, zero
    beyond each motion's own frames as the loader pads them (the second convolution's last step reads two frames past m_lens), m_lens N
    frame counts in 4 .. T (any order) -> (N, 512), row i = motion i.  Sequence i runs m_lens[i] // 4 steps.  As in the reference, T enters
    the result of a motion that fills the batch (4 (m_len // 4) + 2 > T): its last step meets the second convolution's zero padding where a
    longer batch has the first convolution's output over zero frames."""
    if not (torch.is_tensor(motions) and motions.is_cuda):
        raise _lib.SynHipError("embed_motions: motions must be a GPU tensor; the evaluator runs on the HIP kernels only (no CPU fallback)")
    pm, pe = movement_encoder.packed(), motion_encoder.packed()
    width = _lib.SYN_T2M_POSE + 4
    if motions.dim() != 3 or motions.shape[2] != width:
        raise ValueError(f"embed_motions: expected motions (N, T, {width}), got {tuple(motions.shape)}")
    n, t = motions.shape[:2]
    frames = np.asarray(torch.as_tensor(m_lens).tolist(), dtype=np.int64).reshape(-1)
    if n < 1 or t < UNIT_LENGTH or len(frames) != n or frames.min() < UNIT_LENGTH or frames.max() > t:
        raise ValueError(f"embed_motions: {n} motions of {t} frames need N >= 1 lengths in {UNIT_LENGTH} .. {t} (m_lens // {UNIT_LENGTH} "
                         "steps, at least one and at most the movement encoder's output)")
    lens = frames // UNIT_LENGTH
    if lens.max() > conv_len(conv_len(t)):
        raise ValueError(f"embed_motions: {int(frames.max())} frames give more steps than the movement encoder's {conv_len(conv_len(t))}")
    key = (id(pm), id(pe))
    if pe.get("model_key") != key:
        m = _lib.SynT2mModel()
        m.conv1_w, m.conv1_b, m.conv2_w, m.conv2_b, m.out_w, m.out_b = pm["ptr"]
        m.motion_in_w, m.motion_in_b = pe["ptr"]
        m.motion_gru, m.motion_head = pe["gru"], pe["head"]
        pe["model"], pe["model_key"], pe["movement"] = m, key, pm          # (pm kept alive: the struct points into its tensors)
    dev = motions.device
    x = motions.detach().float().contiguous()
    lens_dev, orders = _lengths(pe, _lib.SYN_T2M_MOTION, lens, dev)
    out = torch.empty(n, _lib.SYN_T2M_EMB, device=dev)
    lib, st = _lib.load(), _lib.current_stream(dev)
    for c, order in enumerate(orders):
        i, k = c * CHUNK, len(order)
        _lib.check(lib.syn_t2m_encode_motion(C.byref(pe["model"]), x[i:i + k].data_ptr(), k, t, width, lens_dev[i:i + k].data_ptr(),
                                             order.data_ptr(), _workspace(pe, _lib.SYN_T2M_MOTION, k, t, dev).data_ptr(),
                                             out[i:i + k].data_ptr(), st), "syn_t2m_encode_motion")
    return out


def build_evaluators(opt: dict, state: dict | None = None):
    """utils/t2m_eval_tools.py:807-830: the three modules, loaded strictly from `state` (the checkpoint's dict) or from
    <checkpoints_dir>/<t2m | dataset_name>/text_mot_match/model/finest.tar."""
    movement_enc = MovementConvEncoder(opt["dim_pose"] - 4, opt["dim_movement_enc_hidden"], opt["dim_movement_latent"])
    text_enc = TextEncoderBiGRUCo(word_size=opt["dim_word"], pos_size=opt["dim_pos_ohot"], hidden_size=opt["dim_text_hidden"],
                                  output_size=opt["dim_coemb_hidden"], device=opt["device"])
    motion_enc = MotionEncoderBiGRUCo(input_size=opt["dim_movement_latent"], hidden_size=opt["dim_motion_hidden"],
                                      output_size=opt["dim_coemb_hidden"], device=opt["device"])
    if state is None:
        ckpt_dir = "t2m" if opt["dataset_name"] == "humanml" else opt["dataset_name"]
        state = torch.load(os.path.join(opt["checkpoints_dir"], ckpt_dir, "text_mot_match", "model", "finest.tar"), map_location="cpu")
    movement_enc.load_state_dict(state["movement_encoder"], strict=True)
    text_enc.load_state_dict(state["text_encoder"], strict=True)
    motion_enc.load_state_dict(state["motion_encoder"], strict=True)
    return text_enc, motion_enc, movement_enc


class EvaluatorMDMWrapper(object):
    """utils/t2m_eval_tools.py:833-899.  `checkpoints_dir` replaces the path the reference hard-codes; `state` takes the checkpoint's
    three state dicts ({'movement_encoder', 'text_encoder', 'motion_encoder'}) directly."""

    def __init__(self, dataset_name, device, checkpoints_dir=None, state=None):
        if state is None and checkpoints_dir is None:
            raise ValueError("EvaluatorMDMWrapper: give checkpoints_dir (holding t2m/text_mot_match/model/finest.tar) or state")
        opt = {
            "dataset_name": dataset_name, "device": device, "dim_word": 300, "max_motion_length": 196, "dim_pos_ohot": POS_SIZE,
            "dim_motion_hidden": 1024, "max_text_len": 20, "dim_text_hidden": 512, "dim_coemb_hidden": 512,
            "dim_pose": 623 if dataset_name == "humanml" else 251, "dim_movement_enc_hidden": 512, "dim_movement_latent": 512,
            "checkpoints_dir": checkpoints_dir, "unit_length": UNIT_LENGTH,
        }
        self.text_encoder, self.motion_encoder, self.movement_encoder = build_evaluators(opt, state)
        self.opt = opt
        self.device = opt["device"]
        for m in (self.text_encoder, self.motion_encoder, self.movement_encoder):
            m.to(opt["device"])
            m.eval()

    def _motions(self, motions, m_lens):
        motions = motions.detach().to(self.device).float()
        m_lens = torch.as_tensor(m_lens)
        if motions.dim() != 3 or m_lens.dim() != 1 or motions.shape[0] != m_lens.shape[0] or motions.shape[0] < 1:
            raise ValueError(f"EvaluatorMDMWrapper: expected motions (N, T, D) and N >= 1 lengths, got {tuple(motions.shape)} and "
                             f"{tuple(m_lens.shape)}")
        align_idx = np.argsort(m_lens.data.tolist())[::-1].copy()
        idx = self._index(align_idx, motions.device) if motions.is_cuda else torch.from_numpy(align_idx)
        return align_idx, idx, embed_motions(self.movement_encoder, self.motion_encoder, motions[idx], m_lens[align_idx])

    def _index(self, align_idx: np.ndarray, dev) -> torch.Tensor:
        """The reordering as a device index, cached by value (a graph capture after its warm call uploads nothing)."""
        cache = self.__dict__.setdefault("_syn_index", {})
        key = align_idx.tobytes()
        if key not in cache:
            if len(cache) > 7:
                cache.clear()
            cache[key] = torch.from_numpy(align_idx).to(dev)
        return cache[key]

    def __getstate__(self):
        return engine.drop_caches(self)

    # Please note that the results does not following the order of inputs (the reference's comment: both come back in align_idx order)
    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        with torch.no_grad():
            word_embs = word_embs.detach().to(self.device).float()
            pos_ohot = pos_ohot.detach().to(self.device).float()
            _, idx, motion_embedding = self._motions(motions, m_lens)
            text_embedding = self.text_encoder(word_embs, pos_ohot, cap_lens)
            text_embedding = text_embedding[idx]
        return text_embedding, motion_embedding

    def get_motion_embeddings(self, motions, m_lens):
        with torch.no_grad():
            return self._motions(motions, m_lens)[2]
