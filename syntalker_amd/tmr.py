"""TMR's two ACTOR-style encoders on the HIP stack kernel (include/syn_hip.h: syn_tmr_encode).

The h3d trainer (h3d_diffusion_new_trainer.py:170-176, 370-374) conditions on `style_feature = motionclip(tmr_tar_pose).loc`, and the
prompt path (test_h3d.py) on `textencoder(prompt).loc`.  Both modules here keep the reference's constructor arguments and
state_dict keys (models/temos/motionencoder/actor.py, models/temos/textencoder/distillbert_actor.py), so the reference's
`motion_epoch=299.ckpt` / `text_epoch=299.ckpt` load with strict=True.  The transformer stack (input Linear, distribution tokens,
positional table, 4 post-norm encoder layers, rows 0 / 1 out) runs as HIP kernels; the text encoder's DistilBERT runs on PyTorch by
default (once per prompt batch, frozen) and on HIP kernels too with `text_on_hip=True` (syn_bert_encode: token ids -> last_hidden_state).
Both are frozen inference modules, as in the reference's trainer: train(True) raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib, engine

D, FF, HEADS, LAYERS = 256, 1024, 4, _lib.SYN_TMR_LAYERS
MAX_LEN = _lib.SYN_TMR_MAX_LEN
BERT_D, BERT_HEADS, BERT_FF, BERT_MAX_LAYERS = _lib.SYN_BERT_D, _lib.SYN_BERT_HEADS, _lib.SYN_BERT_FF, _lib.SYN_BERT_MAX_LAYERS
DEFAULT_TEXT_MODEL = "./ckpt/distilbert-base-uncased"         # h3d_diffusion_new_trainer.py:169


def workspace_bytes(n_seq: int, max_len: int) -> int:
    """syn_tmr_encode's workspace (include/syn_hip.h): per row of (max_len + 2) x n_seq, x fp32 256 | qkv bf16 768 | attention fp32 256 |
    FF hidden fp32 1024."""
    return n_seq * (max_len + 2) * (D * 4 + 3 * D * 2 + D * 4 + FF * 4)


def bert_workspace_bytes(n_seq: int, max_len: int) -> int:
    """syn_bert_encode's workspace (include/syn_hip.h): per row of max_len x n_seq, qkv fp32 2304 (reused for a Linear's output before its
    LayerNorm) | attention fp32 768 | FF hidden fp32 3072."""
    return n_seq * max_len * 4 * (3 * BERT_D + BERT_D + BERT_FF)


def _packed_bytes(n: int, k: int) -> int:
    return 4 * n * ((k + 31) // 32 * 32)                       # hi + lo bf16 fragments, k padded to the MFMA's 32


def _check_config(who: str, where: str, vae, latent_dim, ff_size, num_layers, num_heads, activation):
    if not (vae is True and latent_dim == D and ff_size == FF and num_layers == LAYERS and num_heads == HEADS and activation == "gelu"):
        raise NotImplementedError(
            f"{who}: built for the configuration the reference uses ({where}: vae=True, latent_dim 256, ff_size 1024, 4 layers, "
            f"4 heads, gelu), got vae={vae}, latent_dim={latent_dim}, ff_size={ff_size}, num_layers={num_layers}, "
            f"num_heads={num_heads}, activation={activation!r}")


class PositionalEncoding(nn.Module):
    """Sinusoidal table as a (max_len, 1, d) buffer `pe` (models/temos/operator/position_encoding_layer.py): pe[s, 0, 2i] = sin(s w_i),
    pe[s, 0, 2i + 1] = cos(s w_i), w_i = 10000^(-2i / d)."""

    def __init__(self, d_model: int, dropout: float = 0.1, max_len: int = 5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pos = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.register_buffer("pe", pe.unsqueeze(1))


class _TmrStack(nn.Module):
    """What both encoders share: the distribution tokens, the positional table, the encoder stack and the HIP call.  Subclasses
    register their input Linear first (the reference's attribute order, hence its state_dict order) and name it in `_in_linear`."""

    _in_linear = ""
    _relu_in = 0

    def _build_stack(self, dropout: float):
        self.mu_token = nn.Parameter(torch.randn(D))
        self.logvar_token = nn.Parameter(torch.randn(D))
        self.sequence_pos_encoding = PositionalEncoding(D, dropout)
        layer = nn.TransformerEncoderLayer(d_model=D, nhead=HEADS, dim_feedforward=FF, dropout=dropout, activation="gelu")
        self.seqTransEncoder = nn.TransformerEncoder(layer, num_layers=LAYERS, enable_nested_tensor=False)   # parameter container
        super().train(False)

    __getstate__ = engine.drop_caches         # (deepcopy / torch.save: without the packed copy - ctypes pointers into this module's tensors)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} is a frozen inference module here (the reference's trainer keeps it in eval(), "
                                      "h3d_diffusion_new_trainer.py:170-176); training the TMR encoders is not built")
        return super().train(False)

    def _stack_tensors(self):
        return [p for n, p in self.named_parameters() if not n.startswith("text_model.")] + [self.sequence_pos_encoding.pe]

    def packed(self):
        """syn_tmr_model of this module: fragment-packed weights and views of the biases.  Rebuilt when a parameter changes (version
        counters, `engine.weights_key`) or moves."""
        return engine.derived(self, self._stack_tensors(), self._pack)

    def _pack(self, p: dict):
        if not self.mu_token.is_cuda:
            raise _lib.SynHipError(f"{type(self).__name__} runs on the HIP kernels only: move the module to the GPU (no CPU fallback)")
        lib = _lib.load()
        st = _lib.current_stream(self.mu_token.device)
        keep = p["keep"]

        def pack(w):
            w = w.detach().float().contiguous()
            out = torch.empty(_packed_bytes(*w.shape), dtype=torch.uint8, device=w.device)
            _lib.check(lib.syn_tmr_pack_weight(w.data_ptr(), w.shape[0], w.shape[1], out.data_ptr(), st), "syn_tmr_pack_weight")
            keep.extend((w, out))
            return out.data_ptr()

        def vec(t):
            t = t.detach().float().contiguous()
            keep.append(t)
            return t.data_ptr()

        lin = self.get_submodule(self._in_linear)
        m = _lib.SynTmrModel()
        m.nfeats, m.relu_in = lin.in_features, self._relu_in
        m.w_in, m.b_in = pack(lin.weight), vec(lin.bias)
        m.mu_token, m.logvar_token, m.pe = vec(self.mu_token), vec(self.logvar_token), vec(self.sequence_pos_encoding.pe)
        for i, y in enumerate(self.seqTransEncoder.layers):
            a = y.self_attn
            m.layer[i] = _lib.SynTmrLayer(pack(a.in_proj_weight), vec(a.in_proj_bias), pack(a.out_proj.weight), vec(a.out_proj.bias),
                                          vec(y.norm1.weight), vec(y.norm1.bias), pack(y.linear1.weight), vec(y.linear1.bias),
                                          pack(y.linear2.weight), vec(y.linear2.bias), vec(y.norm2.weight), vec(y.norm2.bias))
        p.update(model=m, **self._pack_more(pack, vec))

    def _pack_more(self, pack, vec) -> dict:
        """Further entries of the packed() cache a subclass derives from its weights (`pack`: a Linear's weight -> fragment pointer, `vec`: fp32
        pointer; both keep their tensors alive with the cache)."""
        return {}

    def _encode(self, x: torch.Tensor, lengths):
        """x (B, L, nfeats) on the module's device, lengths None (all L) or a device int tensor (B,) -> (mu, logvar) fp32 (B, 256)."""
        p = self.packed()
        m = p["model"]
        if x.dim() != 3 or x.shape[2] != m.nfeats:
            raise ValueError(f"{type(self).__name__}: expected input (B, L, {m.nfeats}), got {tuple(x.shape)}")
        b, L, _ = x.shape
        if b < 1 or not 1 <= L <= MAX_LEN:
            raise ValueError(f"{type(self).__name__}: {L} rows per sequence; the HIP stack takes 1 .. {MAX_LEN} (+ the two distribution "
                             f"tokens = 256 attention rows), batch >= 1")
        if x.device != self.mu_token.device:
            raise ValueError(f"input on {x.device}, module on {self.mu_token.device}")
        x = x.detach().float().contiguous()
        if lengths is not None:
            lengths = lengths.to(device=x.device, dtype=torch.int32).contiguous()
            if lengths.shape != (b,):
                raise ValueError(f"lengths: expected ({b},), got {tuple(lengths.shape)}")
        ws = engine.workspace(p["ws"], (b, L), workspace_bytes(b, L), x.device)
        mu = torch.empty(b, D, device=x.device)
        logvar = torch.empty(b, D, device=x.device)
        _lib.check(_lib.load().syn_tmr_encode(C.byref(m), x.data_ptr(), b, L, _lib.ptr(lengths), ws.data_ptr(),
                                              mu.data_ptr(), logvar.data_ptr(), _lib.current_stream(x.device)), "syn_tmr_encode")
        return mu, logvar

    @staticmethod
    def _normal(mu, logvar):
        return torch.distributions.Normal(mu, logvar.exp().pow(0.5))


class ActorAgnosticEncoder(_TmrStack):
    """models/temos/motionencoder/actor.py's encoder: features (B, L, nfeats) -> Normal(mu, exp(logvar) ** 0.5), each (B, 256)."""

    _in_linear = "skel_embedding"

    def __init__(self, nfeats: int, vae: bool = True, latent_dim: int = 256, ff_size: int = 1024, num_layers: int = 4,
                 num_heads: int = 4, dropout: float = 0.1, activation: str = "gelu", **kwargs):
        super().__init__()
        _check_config("ActorAgnosticEncoder", "h3d_diffusion_new_trainer.py:174", vae, latent_dim, ff_size, num_layers, num_heads, activation)
        if not 1 <= nfeats <= _lib.SYN_TMR_MAX_FEATS:
            raise NotImplementedError(f"ActorAgnosticEncoder: nfeats {nfeats} outside 1 .. {_lib.SYN_TMR_MAX_FEATS}")
        self.nfeats = nfeats
        self.skel_embedding = nn.Linear(nfeats, D)
        self._build_stack(dropout)

    def encode(self, features: torch.Tensor, lengths=None, max_len=None):
        """(mu, logvar), each (B, 256).  No host synchronisation when `lengths` is None or a device tensor: capturable in a CUDA graph.
        A captured encode replays against the packed weights and the workspace of its capture: while the graph is in use, keep the
        parameters unwritten (a write re-packs into new buffers and frees the old ones) and do not encode more than five other shapes
        on this module (the workspace cache drops its buffers beyond that)."""
        b, t = features.shape[0], features.shape[1]
        if lengths is not None and not torch.is_tensor(lengths):
            lengths = [int(v) for v in lengths]
            width = max_len if max_len else max(lengths)
            lengths = torch.tensor(lengths, dtype=torch.int32)
        else:                 # (a device tensor's maximum is not read back: no host synchronisation)
            width = max_len if max_len else t
        if width != t:        # the reference concatenates a (B, 2 + width) mask against 2 + t rows: only width == t runs there
            raise ValueError(f"ActorAgnosticEncoder: mask width {width} (max_len or max(lengths)) must equal the {t} input rows")
        if lengths is not None and lengths.shape[0] != b:
            raise ValueError(f"ActorAgnosticEncoder: {lengths.shape[0]} lengths for {b} sequences")
        return self._encode(features, lengths)

    def forward(self, features: torch.Tensor, lengths=None, max_len=None):
        return self._normal(*self.encode(features, lengths, max_len))


class DistilbertActorAgnosticEncoder(_TmrStack):
    """models/temos/textencoder/distillbert_actor.py's encoder: prompt(s) -> DistilBERT (frozen) -> ReLU + Linear(768 -> 256) and the HIP
    stack -> Normal(mu, exp(logvar) ** 0.5), each (B, 256).  `modelpath` is a local directory (tokenizer + config + weights).

    `text_on_hip=False` (default): DistilBERT is transformers' module on PyTorch.  `text_on_hip=True`: tokenizer (host) -> ids ->
    syn_bert_encode -> syn_tmr_encode, no torch.nn module in between.  The `text_model` submodule and the state_dict are the same either way
    (the reference's text_epoch=299.ckpt loads with strict=True); its parameters are what the packed copy is built from, in the same
    packed() cache and under the same staleness key (load_state_dict, an in-place write or .to() re-pack).  The packed copy costs 4 bytes
    per Linear weight (hi + lo bf16 fragments) beside the fp32 originals: about 170 MB for the six layers of distilbert-base-uncased.
    The HIP path takes a length per prompt, `attention_mask.sum(1)`: the tokenizer pads on the right, so a mask is a prefix of ones; a mask
    with holes is not expressible on this path.  It is built for dim 768, 12 heads, hidden_dim 3072, gelu and 1 .. 12 layers (learned or
    sinusoidal position table); any other configuration raises NotImplementedError at construction."""

    _in_linear = "projection.1"
    _relu_in = 1

    def __init__(self, modelpath: str, finetune: bool = False, vae: bool = True, latent_dim: int = 256, ff_size: int = 1024,
                 num_layers: int = 4, num_heads: int = 4, dropout: float = 0.1, activation: str = "gelu", text_on_hip: bool = False,
                 **kwargs):
        super().__init__()
        _check_config("DistilbertActorAgnosticEncoder", "h3d_diffusion_new_trainer.py:171", vae, latent_dim, ff_size, num_layers,
                      num_heads, activation)
        if finetune:
            raise NotImplementedError("DistilbertActorAgnosticEncoder: finetune=True (training DistilBERT) is not built; the reference's "
                                      "trainer uses the frozen default (h3d_diffusion_new_trainer.py:171)")
        from transformers import AutoModel, AutoTokenizer, logging     # only the text encoder needs transformers
        logging.set_verbosity_error()
        os.environ.setdefault("TOKENIZERS_PARALLELISM", "false")
        self.tokenizer = AutoTokenizer.from_pretrained(modelpath, local_files_only=True)
        self.text_model = AutoModel.from_pretrained(modelpath, local_files_only=True)
        for p in self.text_model.parameters():
            p.requires_grad = False
        self.text_on_hip = bool(text_on_hip)
        if self.text_on_hip:
            self._check_text_config(self.text_model.config)
        self.text_encoded_dim = self.text_model.config.hidden_size
        self.projection = nn.Sequential(nn.ReLU(), nn.Linear(self.text_encoded_dim, D))
        self._build_stack(dropout)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """As nn.Module's; a checkpoint saved under a transformers release that kept DistilBERT's `embeddings.position_ids` as a persistent
        buffer carries that key (a fixed arange the model rebuilds itself): it is dropped when this model does not have it."""
        key = "text_model.embeddings.position_ids"
        if key in state_dict and key not in self.state_dict():
            state_dict = {k: v for k, v in state_dict.items() if k != key}
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    @staticmethod
    def _check_text_config(cfg):
        want = (("dim", BERT_D), ("n_heads", BERT_HEADS), ("hidden_dim", BERT_FF), ("activation", "gelu"))
        for field, value in want:
            if getattr(cfg, field, None) != value:
                raise NotImplementedError(f"DistilbertActorAgnosticEncoder(text_on_hip=True): the HIP DistilBERT is built for {field} = {value!r}, "
                                          f"the model's config has {field} = {getattr(cfg, field, None)!r}")
        if not 1 <= getattr(cfg, "n_layers", 0) <= BERT_MAX_LAYERS:
            raise NotImplementedError(f"DistilbertActorAgnosticEncoder(text_on_hip=True): n_layers = {getattr(cfg, 'n_layers', None)!r} outside "
                                      f"1 .. {BERT_MAX_LAYERS}")

    def _stack_tensors(self):
        if not self.text_on_hip:
            return super()._stack_tensors()
        return list(self.parameters()) + [self.sequence_pos_encoding.pe]

    def _pack_more(self, pack, vec) -> dict:
        if not self.text_on_hip:
            return {}
        t = self.text_model
        emb = t.embeddings
        m = _lib.SynBertModel()
        m.n_layers, m.vocab, m.n_pos = len(t.transformer.layer), emb.word_embeddings.weight.shape[0], emb.position_embeddings.weight.shape[0]
        m.word, m.pos = vec(emb.word_embeddings.weight), vec(emb.position_embeddings.weight)
        m.emb_ln_g, m.emb_ln_b = vec(emb.LayerNorm.weight), vec(emb.LayerNorm.bias)
        for i, y in enumerate(t.transformer.layer):
            a, f = y.attention, y.ffn
            m.layer[i] = _lib.SynBertLayer(pack(torch.cat([a.q_lin.weight, a.k_lin.weight, a.v_lin.weight]).detach()),
                                           vec(torch.cat([a.q_lin.bias, a.k_lin.bias, a.v_lin.bias])),
                                           pack(a.out_lin.weight), vec(a.out_lin.bias), vec(y.sa_layer_norm.weight), vec(y.sa_layer_norm.bias),
                                           pack(f.lin1.weight), vec(f.lin1.bias), pack(f.lin2.weight), vec(f.lin2.bias),
                                           vec(y.output_layer_norm.weight), vec(y.output_layer_norm.bias))
        return {"bert": m, "bert_ws": {}}

    def tokenize(self, texts):
        """(input ids, attention mask) as the reference's tokenizer call makes them (padding=True), on the module's device."""
        ids, mask = self._tokenize_host(texts)
        dev = self.mu_token.device
        return ids.to(dev), mask.to(dev)

    def _tokenize_host(self, texts):
        enc = self.tokenizer([texts] if isinstance(texts, str) else list(texts), return_tensors="pt", padding=True)
        return enc["input_ids"], enc["attention_mask"]

    def hidden_states(self, ids: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """DistilBERT's last_hidden_state on the HIP kernels (text_on_hip=True only): ids (B, L) and lengths (B,), int tensors on the module's
        device -> (B, L, 768) fp32 with rows at or beyond a prompt's length exactly zero.  No host synchronisation, so ids are not range-checked
        here: the kernel clamps them into the table, `encode` checks them on the host where they originate."""
        if not self.text_on_hip:
            raise _lib.SynHipError("DistilbertActorAgnosticEncoder: hidden_states / encode_ids run the HIP DistilBERT; build the module with text_on_hip=True")
        p = self.packed()
        if ids.dim() != 2:
            raise ValueError(f"DistilbertActorAgnosticEncoder: expected ids (B, L), got {tuple(ids.shape)}")
        b, L = ids.shape
        if b < 1 or b > _lib.SYN_TMR_MAX_SEQ or not 1 <= L <= MAX_LEN:
            raise ValueError(f"DistilbertActorAgnosticEncoder: ids {tuple(ids.shape)}; the HIP path takes 1 .. {MAX_LEN} tokens per prompt "
                             f"and 1 .. {_lib.SYN_TMR_MAX_SEQ} prompts")
        if L > p["bert"].n_pos:
            raise ValueError(f"DistilbertActorAgnosticEncoder: {L} tokens per prompt, the model has {p['bert'].n_pos} positions")
        dev = self.mu_token.device
        if ids.device != dev or lengths.device != dev:
            raise ValueError(f"ids on {ids.device}, lengths on {lengths.device}, module on {dev}")
        if lengths.shape != (b,):
            raise ValueError(f"lengths: expected ({b},), got {tuple(lengths.shape)}")
        ids = ids.to(torch.int32).contiguous()
        lengths = lengths.to(torch.int32).contiguous()
        ws = engine.workspace(p["bert_ws"], (b, L), bert_workspace_bytes(b, L), dev)
        hidden = torch.empty(b, L, BERT_D, device=dev)
        _lib.check(_lib.load().syn_bert_encode(C.byref(p["bert"]), ids.data_ptr(), b, L, lengths.data_ptr(), ws.data_ptr(), hidden.data_ptr(),
                                               _lib.current_stream(dev)), "syn_bert_encode")
        return hidden

    def encode_ids(self, ids: torch.Tensor, lengths: torch.Tensor):
        """(mu, logvar), each (B, 256), from token ids (B, L) and lengths (B,) on the module's device (text_on_hip=True only): syn_bert_encode ->
        syn_tmr_encode.  No host synchronisation: capturable in a CUDA graph, under `ActorAgnosticEncoder.encode`'s conditions."""
        return self._encode(self.hidden_states(ids, lengths), lengths)

    def encode(self, texts):
        """(mu, logvar), each (B, 256), for a str (B = 1) or a list of str."""
        if self.text_on_hip:
            ids, mask = self._tokenize_host(texts)
            vocab = self.text_model.embeddings.word_embeddings.weight.shape[0]
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
                raise ValueError(f"DistilbertActorAgnosticEncoder: token id outside 0 .. {vocab - 1} (tokenizer and model do not match)")
            dev = self.mu_token.device
            return self.encode_ids(ids.to(dev), mask.sum(1, dtype=torch.int32).to(dev))
        ids, mask = self.tokenize(texts)
        with torch.no_grad():
            hidden = self.text_model(input_ids=ids, attention_mask=mask).last_hidden_state
        return self._encode(hidden, mask.sum(1, dtype=torch.int32))

    def forward(self, texts):
        return self._normal(*self.encode(texts))


def build_encoders(args, device="cuda", text: bool = True):
    """(motion encoder, text encoder or None) as h3d_diffusion_new_trainer.py:168-176 builds them: ActorAgnosticEncoder(623) and
    DistilbertActorAgnosticEncoder(`tmr_text_model_path` or ./ckpt/distilbert-base-uncased), loaded from `tmr_base_path`'s
    motion_epoch=299.ckpt / text_epoch=299.ckpt.  A configured path that does not exist raises; an unset or empty key leaves the
    random initialisation.  `tmr_text_on_hip: true` in the configuration builds the text encoder with DistilBERT on the HIP kernels."""
    from .config import _require
    base = getattr(args, "tmr_base_path", None)
    if base:
        _require(base, "tmr_base_path")
    motion = ActorAgnosticEncoder(nfeats=623, vae=True, num_layers=4)
    if base:
        motion.load_state_dict(torch.load(os.path.join(base, "motion_epoch=299.ckpt"), map_location="cpu"))
    enc_text = None
    if text:
        path = getattr(args, "tmr_text_model_path", None) or DEFAULT_TEXT_MODEL
        _require(path, "tmr_text_model_path")
        enc_text = DistilbertActorAgnosticEncoder(path, num_layers=4, text_on_hip=bool(getattr(args, "tmr_text_on_hip", False)))
        if base:
            enc_text.load_state_dict(torch.load(os.path.join(base, "text_epoch=299.ckpt"), map_location="cpu"))
        enc_text = enc_text.to(device)
    return motion.to(device), enc_text
