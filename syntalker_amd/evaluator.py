"""The reference's FGD motion embedder, `VAESKConv` (models/motion_representation.py:67-75), on the HIP skeleton-conv kernels
(include/syn_hip.h: syn_skel_encode).

The reference's `test()` embeds every take with `eval_copy.map2latent` (diffusion_rvqvae_trainer.py:613-619, 718), loaded from
`weights/AESKConv_240_100.bin` (configs/diffusion_rvqvae_128.yaml:8-10).  With `variational: False` (every config) map2latent is
`LocalEncoder(x)` (models/motion_encoder.py:698-787): four `SkeletonResidual` layers (models/utils/skeleton.py:547-586) over the SMPL-X
edge graph,

    r   = GroupNorm(10, C_out)( conv1d(x, W*M, b, kernel 4, stride 2, zero pad 1) )
    s   = conv1d(x, Ws*Ms, bs, kernel 1, stride 2)
    out = tanh( P @ (r + s) )                       P: mean pooling along the kinematic chains, where it changes the edge count

This module keeps the reference's constructor and all 56 state_dict keys (the VQDecoderV3 decoder and fc_mu / fc_logvar are held, never
run), so the checkpoint loads strictly.  The topology is restated from the reference's skeleton.py (`build_edge_topology` :316,
`calc_edge_mat` / `find_neighbor` :373-420, `SkeletonPool` :162-235); the masks and pooling matrices that run are the loaded parameters.
Eval-only, like the TMR encoders.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
from torch import nn

from . import _lib, engine

CHANNEL_BASE, KERNEL, SKELETON_DIST, GROUPS, EPS = 6, 4, 2, 10, 1e-5     # LocalEncoder's fixed settings (motion_encoder.py:701-713)
LAYERS = _lib.SYN_SKEL_LAYERS
TILE = 16                                                                 # output frames per workgroup of the HIP kernels
SMPLX_FILE = "smplx_models/smplx/SMPLX_NEUTRAL_2020.npz"                 # under args.data_path_1 (motion_representation.py:70)


# ---- topology (models/utils/skeleton.py) --------------------------------------------------------------------------------------------

def build_edge_topology(parents) -> list[tuple[int, int]]:
    """skeleton.py:316: a virtual edge (0, J) for the root, then (parent, i) for every other joint."""
    j = len(parents)
    return [(0, j)] + [(int(parents[i]), i) for i in range(1, j)]


def edge_distances(edges) -> np.ndarray:
    """calc_edge_mat (skeleton.py:373-397): 0 on the diagonal, 1 between edges that share a joint, shortest paths over those."""
    e = np.asarray(edges)
    share = (e[:, None, :, None] == e[None, :, None, :]).any(axis=(2, 3))
    d = np.where(share, 1, 100000).astype(np.int64)
    np.fill_diagonal(d, 0)
    for k in range(len(e)):
        d = np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :])
    return d


def find_neighbor(edges, dist: int) -> list[list[int]]:
    """skeleton.py:400-420: for each edge, the edges within `dist` (itself included), in index order."""
    d = edge_distances(edges)
    return [[int(j) for j in np.nonzero(row <= dist)[0]] for row in d]


def pool_edges(edges, last_pool: bool):
    """SkeletonPool's chain walk and pairing (skeleton.py:162-209): (pooling_list, new_edges).  Chains run from the root or a joint of
    degree > 2 to a leaf or the next such joint; each chain is pooled in pairs from its far end (a lone first edge stays alone), or whole
    in the last layer (`last_pool`)."""
    degree = [0] * (max(max(e) for e in edges) + 1)
    for a, b in edges:
        degree[a] += 1
        degree[b] += 1
    chains = []

    def walk(j, seq):
        if degree[j] > 2 and j != 0:
            chains.append(seq)
            seq = []
        if degree[j] == 1:
            chains.append(seq)
            return
        for idx, (a, b) in enumerate(edges):
            if a == j:
                walk(b, seq + [idx])

    walk(0, [])
    pooling, new_edges = [], []
    for seq in chains:
        if last_pool:
            pooling.append(seq)
            continue
        if len(seq) % 2 == 1:
            pooling.append([seq[0]])
            new_edges.append(edges[seq[0]])
            seq = seq[1:]
        for i in range(0, len(seq), 2):
            pooling.append([seq[i], seq[i + 1]])
            new_edges.append((edges[seq[i]][0], edges[seq[i + 1]][1]))
    return pooling, new_edges


def pool_matrix(pooling, n_edges: int, per_edge: int) -> torch.Tensor:
    """SkeletonPool.weight (skeleton.py:223-229): output channel (i, c) is the mean of channel c of the edges in pooling[i]."""
    w = torch.zeros(len(pooling) * per_edge, n_edges * per_edge)
    for i, group in enumerate(pooling):
        for j in group:
            for c in range(per_edge):
                w[i * per_edge + c, j * per_edge + c] = 1.0 / len(group)
    return w


def layer_plan(parents, grow, vae_length: int) -> list[dict]:
    """Each layer's topology and widths, as LocalEncoder.__init__ derives them (motion_encoder.py:729-768): edges, neighbour lists,
    C_in, C_out, the pooling (None where it keeps the edge count, so the reference appends no pool module) and the output width."""
    if len(grow) != LAYERS:
        raise ValueError(f"vae_grow: the HIP encoder is built for {LAYERS} layers (vae_layer 4), got {len(grow)} growth factors")
    edges, base, plan = build_edge_topology(parents), CHANNEL_BASE, []
    for i in range(LAYERS):
        nb = find_neighbor(edges, SKELETON_DIST)
        cin, cout = base * len(edges), base * int(grow[i]) * len(edges)
        per_edge = cout // len(nb)
        pooling, new_edges = pool_edges(edges, last_pool=i == LAYERS - 1)
        pooled = len(pooling) != len(edges)
        if cout % GROUPS:
            raise ValueError(f"layer {i}: GroupNorm({GROUPS}, {cout}) needs a width divisible by {GROUPS}")
        plan.append(dict(edges=edges, neighbours=nb, cin=cin, cout=cout, per_edge=per_edge, pooling=pooling if pooled else None,
                         out_width=len(pooling) * per_edge if pooled else cout))
        edges, base = new_edges, base * int(grow[i])
    if plan[-1]["out_width"] != vae_length:
        raise ValueError(f"the skeleton tree ends at {plan[-1]['out_width']} channels, vae_length is {vae_length}")
    return plan


def read_parents(args) -> np.ndarray:
    """kintree_table[0] of the SMPL-X model the reference reads (motion_representation.py:70-72)."""
    smpl = np.load(args.data_path_1 + SMPLX_FILE, encoding="latin1")
    return smpl["kintree_table"][0].astype(np.int32)


# ---- modules with the reference's parameter layout ------------------------------------------------------------------------------------

class SkeletonConv(nn.Module):
    """skeleton.py:9-110 without the offset branch: parameters `mask` (neighbour mask, frozen), `weight`, `bias`, in that order."""

    def __init__(self, neighbours, cin: int, cout: int, kernel: int):
        super().__init__()
        n = len(neighbours)
        ci, co = cin // n, cout // n
        mask = torch.zeros(cout, cin, kernel)
        for i, nb in enumerate(neighbours):
            cols = [k * ci + c for k in nb for c in range(ci)]
            mask[co * i: co * (i + 1), cols] = 1
        self.mask = nn.Parameter(mask, requires_grad=False)
        w = torch.empty(cout, cin, kernel)
        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
        self.weight = nn.Parameter(w * mask)
        self.bias = nn.Parameter(torch.zeros(cout))


class SkeletonPool(nn.Module):
    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)


class SkeletonResidual(nn.Module):
    """skeleton.py:547-586 with extra_conv 0: residual = (SkeletonConv k4 s2, GroupNorm(10)), shortcut = SkeletonConv k1 s2,
    common = ([SkeletonPool,] Tanh)."""

    def __init__(self, p: dict):
        super().__init__()
        self.residual = nn.Sequential(SkeletonConv(p["neighbours"], p["cin"], p["cout"], KERNEL), nn.GroupNorm(GROUPS, p["cout"]))
        self.shortcut = SkeletonConv(p["neighbours"], p["cin"], p["cout"], 1)
        common = [] if p["pooling"] is None else [SkeletonPool(pool_matrix(p["pooling"], len(p["edges"]), p["per_edge"]))]
        self.common = nn.Sequential(*common, nn.Tanh())


class LocalEncoder(nn.Module):
    def __init__(self, plan):
        super().__init__()
        self.layers = nn.ModuleList(nn.Sequential(SkeletonResidual(p)) for p in plan)


class ResBlock(nn.Module):
    """models/utils/layer.py:203-216 (parameters only)."""

    def __init__(self, ch: int):
        super().__init__()
        self.model = nn.Sequential(nn.Conv1d(ch, ch, 3, 1, 1), nn.LeakyReLU(0.2), nn.Conv1d(ch, ch, 3, 1, 1))


class VQDecoderV3(nn.Module):
    """motion_encoder.py:299-332, held for the checkpoint's keys only: `decode` is not built."""

    def __init__(self, args):
        super().__init__()
        n_up, length, dim = int(args.vae_layer), int(args.vae_length), int(args.vae_test_dim)
        ch = [length] * n_up + [dim]
        layers = [] if length == ch[0] else [nn.Conv1d(length, ch[0], 3, 1, 1)]
        layers += [ResBlock(ch[0]), ResBlock(ch[0])]
        for i in range(n_up):
            layers += [nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv1d(ch[i], ch[i + 1], 3, 1, 1), nn.LeakyReLU(0.2)]
        layers += [nn.Conv1d(ch[-1], ch[-1], 3, 1, 1)]
        self.main = nn.Sequential(*layers)


# ---- the packed model and the HIP call ---------------------------------------------------------------------------------------------

def _round(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def workspace_bytes(layers, n_clips: int, n_frames: int) -> int:
    """syn_skel_encode's workspace (include/syn_hip.h): per layer, pre-norm r | s fp32 [n_clips][T][2 roundup(C_out, 16)] and the
    GroupNorm partial sums fp64 [n_clips][ceil(T / 16)][10][2], T = n_frames >> (layer + 1), each region rounded up to 256 bytes."""
    total = 0
    for i, cout in enumerate(layers):
        t = n_frames >> (i + 1)
        total += _round(n_clips * t * 2 * _round(cout, 16) * 4, 256) + _round(n_clips * ((t + TILE - 1) // TILE) * GROUPS * 2 * 8, 256)
    return total


class VAESKConv(nn.Module):
    """models/motion_representation.py:67-75: `map2latent(x)` (B, n, 330) 6D poses -> (B, n / 16, 240), on the HIP kernels."""

    def __init__(self, args):
        super().__init__()
        self.variational = bool(getattr(args, "variational", False))
        self.vae_length = int(args.vae_length)
        self.plan = layer_plan(read_parents(args), list(args.vae_grow), self.vae_length)
        self.in_width = self.plan[0]["cin"]
        self.encoder = LocalEncoder(self.plan)
        self.decoder = VQDecoderV3(args)
        self.fc_mu = nn.Linear(self.vae_length, self.vae_length)
        self.fc_logvar = nn.Linear(self.vae_length, self.vae_length)
        super().train(False)

    __getstate__ = engine.drop_caches         # (deepcopy / torch.save: without the packed copy - ctypes pointers into this module's tensors)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("VAESKConv is the FGD evaluator, an inference module here (the reference's trainer only calls "
                                      "eval_copy.map2latent, diffusion_rvqvae_trainer.py:618-619); training it is not built")
        return super().train(False)

    def decode(self, pre_latent):
        raise NotImplementedError("VAESKConv.decode (models/motion_representation.py:62-64, VQDecoderV3) is not built: the decoder is held "
                                  "for the checkpoint's keys only; the FGD needs map2latent alone")

    def _encoder_tensors(self):
        return list(self.encoder.parameters())

    def packed(self):
        """syn_skel_model of this module: per layer the masked, block-sparse weight fragments of both branches, the biases, GroupNorm affine
        and output pooling as gather lists.  Rebuilt when an encoder parameter changes (version counters, `engine.weights_key`) or moves."""
        return engine.derived(self, self._encoder_tensors(), self._pack)

    def _pack(self, p: dict):
        dev = self.encoder.layers[0][0].shortcut.weight.device
        if dev.type != "cuda":
            raise _lib.SynHipError("VAESKConv runs on the HIP kernels only: move the module to the GPU (no CPU fallback)")
        lib = _lib.load()
        st = _lib.current_stream(dev)
        keep, kept = p["keep"], []
        m = _lib.SynSkelModel()
        for i, seq in enumerate(self.encoder.layers):
            blk = seq[0]
            conv, gn, sc = blk.residual[0], blk.residual[1], blk.shortcut
            cout, cin = conv.weight.shape[0], conv.weight.shape[1]
            cin_p, cout_p = _round(cin, 4), _round(cout, 16)
            f32 = lambda t: t.detach().float().contiguous()
            w, mk, ws, ms = f32(conv.weight), f32(conv.mask), f32(sc.weight), f32(sc.mask)
            # kept K chunks: for each tile of 16 output columns (r columns 0 .. cout_p, s columns cout_p .. 2 cout_p), the chunks of 4
            # consecutive input channels at one tap (k = tap * cin_p + c) that hold a nonzero of W*M / Ws*Ms
            nz = torch.zeros(2 * cout_p, KERNEL, cin_p, dtype=torch.bool, device=dev)
            nz[:cout, :, :cin] = (w * mk).permute(0, 2, 1) != 0
            nz[cout_p:cout_p + cout, 1, :cin] = (ws * ms)[:, :, 0] != 0
            hit = nz.view(2 * cout_p // 16, 16, KERNEL, cin_p // 4, 4).any(4).any(1).flatten(1).cpu()    # (n_tiles, 4 cin_p / 4)
            counts = hit.sum(1)
            off = torch.zeros(hit.shape[0] + 1, dtype=torch.int32)
            off[1:] = torch.cumsum(counts, 0)
            idx = hit.nonzero()[:, 1]
            tap, c0 = idx // (cin_p // 4), idx % (cin_p // 4) * 4
            chunk = ((tap << 16) | c0).to(torch.int32)
            kept.append(float(hit.float().mean()))
            off, chunk = off.to(dev), chunk.to(dev)
            out = torch.empty(max(int(off[-1]), 1) * 64, dtype=torch.float32, device=dev)
            _lib.check(lib.syn_skel_pack_weight(w.data_ptr(), mk.data_ptr(), ws.data_ptr(), ms.data_ptr(), cout, cin, off.data_ptr(),
                                                chunk.data_ptr(), out.data_ptr(), st), "syn_skel_pack_weight")
            bias = torch.zeros(2 * cout_p, dtype=torch.float32, device=dev)
            bias[:cout], bias[cout_p:cout_p + cout] = f32(conv.bias), f32(sc.bias)
            src, sw = self._pool_gather(blk, cout, dev)
            g, b = f32(gn.weight), f32(gn.bias)
            keep += [w, mk, ws, ms, off, chunk, out, bias, g, b, src, sw]
            m.layer[i] = _lib.SynSkelLayer(out.data_ptr(), off.data_ptr(), chunk.data_ptr(), bias.data_ptr(), g.data_ptr(), b.data_ptr(),
                                           src.data_ptr(), sw.data_ptr(), cin, cout, src.shape[0], 0)
        p.update(model=m, kept=kept)

    @staticmethod
    def _pool_gather(blk, cout: int, dev):
        """The layer's output map as gather lists: output channel o = sum_k w[o][k] * channel src[o][k] (src -1: none), from the loaded
        pooling matrix (identity where the layer does not pool)."""
        k_max = _lib.SYN_SKEL_POOL_MAX
        if isinstance(blk.common[0], SkeletonPool):
            pm = blk.common[0].weight.detach().float().cpu()
            if pm.shape[1] != cout:
                raise ValueError(f"pooling matrix {tuple(pm.shape)} does not take the layer's {cout} channels")
            nnz = (pm != 0).sum(1)
            if int(nnz.max()) > k_max:
                raise NotImplementedError(f"a pooled channel averages {int(nnz.max())} inputs; the HIP kernel takes at most {k_max}")
            src = torch.full((pm.shape[0], k_max), -1, dtype=torch.int32)
            sw = torch.zeros(pm.shape[0], k_max)
            for o in range(pm.shape[0]):
                cols = torch.nonzero(pm[o]).flatten()
                src[o, :len(cols)] = cols.to(torch.int32)
                sw[o, :len(cols)] = pm[o, cols]
        else:
            src = torch.full((cout, k_max), -1, dtype=torch.int32)
            src[:, 0] = torch.arange(cout, dtype=torch.int32)
            sw = torch.zeros(cout, k_max)
            sw[:, 0] = 1.0
        return src.to(dev), sw.to(dev)

    def kept_fraction(self) -> list[float]:
        """Per layer, the fraction of (16-column tile, 4-wide K chunk) blocks the kernel runs (of both branches' 2 C_out x 4 C_in)."""
        return list(self.packed()["kept"])

    def map2latent(self, inputs: torch.Tensor) -> torch.Tensor:
        """(B, n, 330) fp32 6D poses on the GPU, n a positive multiple of 16 -> (B, n / 16, 240) = LocalEncoder(inputs).  Five launches, no
        allocation beyond the output (the workspace is cached per shape) and no host synchronisation: capturable in a CUDA graph.  A captured
        call replays against the packed weights and workspace of its capture: keep the encoder's parameters unwritten while the graph is in
        use, and do not embed more than five other shapes on this module."""
        if self.variational:
            raise NotImplementedError("variational=True draws torch.randn_like in map2latent (models/utils/layer.py:117-120); no config sets "
                                      "it and the FGD evaluator is built for variational: False")
        if not inputs.is_cuda:
            raise _lib.SynHipError(f"VAESKConv.map2latent: input on {inputs.device}; the evaluator runs on the HIP kernels only "
                                   "(no CPU fallback)")
        if inputs.dim() != 3 or inputs.shape[2] != self.in_width:
            raise ValueError(f"VAESKConv.map2latent: expected (B, n, {self.in_width}), got {tuple(inputs.shape)}")
        b, n, _ = inputs.shape
        if b < 1 or n < 16 or n % 16:
            raise ValueError(f"VAESKConv.map2latent: n = {n} frames; the four stride-2 layers need a positive multiple of 16 (the reference's "
                             f"branches disagree in length otherwise), batch {b} >= 1")
        p = self.packed()
        dev = inputs.device
        x = inputs.detach().float().contiguous()
        ws = engine.workspace(p["ws"], (b, n), lambda: workspace_bytes([q["cout"] for q in self.plan], b, n), dev)
        out = torch.empty(b, n // 16, self.plan[-1]["out_width"], device=dev)
        _lib.check(_lib.load().syn_skel_encode(C.byref(p["model"]), x.data_ptr(), b, n, ws.data_ptr(), out.data_ptr(),
                                               _lib.current_stream(dev)), "syn_skel_encode")
        return out

    def forward(self, inputs):
        raise NotImplementedError("VAESKConv.forward reconstructs poses through the decoder (not built); the FGD uses map2latent")
