"""ctypes binding of libsyn_hip.so (C ABI: include/syn_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``syntalker_amd/csrc/build.sh`` with
``hipcc --offload-arch=gfx950``.  There is NO fallback: if the shared object is missing or an entry
point fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SYN_HIP_LIB") or os.path.join(_HERE, "csrc", "libsyn_hip.so")   # env override: kernel A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "syn_hip.h")      # the C ABI: the ctypes signatures below are read from it

SYN_LAYERS = 8
ABI_VERSION = 9             # include/syn_hip.h SYN_ABI_VERSION: a library built from other sources is refused at load time
vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64


class SynLayer(C.Structure):
    _fields_ = [("ln1_g", vp), ("ln1_b", vp), ("w_qkv", vp), ("w_proj", vp), ("b_proj", vp),
                ("ln2_g", vp), ("ln2_b", vp), ("w_fc1", vp), ("b_fc1", vp), ("w_fc2", vp), ("b_fc2", vp)]


class SynTrainBlockSave(C.Structure):
    _fields_ = [(n, vp) for n in ("h_attn", "mean_attn", "rstd_attn", "qkv", "xt_ln1", "xt_attn", "h_mlp", "mean_mlp", "rstd_mlp", "pre", "xt_ln2", "xt_gelu")]


class SynTrainStack(C.Structure):
    _fields_ = [("h_in", vp), ("h_out", vp), ("layer", SynLayer * SYN_LAYERS), ("save", SynTrainBlockSave * SYN_LAYERS), ("drop_path", vp),
                ("n_seq", i32), ("reserved", i32), ("sync", vp), ("xch", vp)]


class SynTrainBlockGrad(C.Structure):
    _fields_ = [(n, vp) for n in ("dyt_fc2", "dyt_fc1", "dyt_proj", "dyt_qkv", "part", "dw_fc2", "dw_fc1", "dw_proj", "dw_qkv",
                                   "d_ln2_g", "d_ln2_b", "d_fc2_b", "d_fc1_b", "d_ln1_g", "d_ln1_b", "d_proj_b")]


class SynTrainStackGrad(C.Structure):
    _fields_ = [("fwd", C.POINTER(SynTrainStack)), ("dh_out", vp), ("dh_in", vp), ("layer_t", SynLayer * SYN_LAYERS), ("grad", SynTrainBlockGrad * SYN_LAYERS),
                ("stash", vp), ("first_block", i32), ("last_block", i32)]


class SynModel(C.Structure):
    _fields_ = [("w_in", vp), ("te", vp), ("n_te", i32), ("rot_cos", vp), ("rot_sin", vp),
                ("layer", SynLayer * SYN_LAYERS), ("w_out", vp), ("b_out", vp),
                ("tape", vp), ("tape_bias", vp), ("tape_chunks", i32)]


class SynStep(C.Structure):
    _fields_ = [("n_clips", i32), ("n_variants", i32), ("m_tile", i32), ("reserved", i32),
                ("cond", vp), ("t_model", vp), ("cfg_w", vp),
                ("x_t", vp), ("x_t_bf16", vp), ("noise", vp), ("rng", vp), ("coef", vp), ("t_coef", vp),
                ("x_next", vp), ("x_next_bf16", vp), ("pred_x0", vp),
                ("ws_h", vp), ("ws_xn", vp), ("ws_q", vp), ("ws_k", vp), ("ws_vt", vp), ("ws_o", vp),
                ("ws_hid", vp), ("ws_hc", vp), ("ws_sync", vp), ("ws_x0v", vp), ("ws_xch", vp),
                ("x_fragment_order", i32), ("cfg_w_clip_stride", i32)]


class SynEdit(C.Structure):
    """include/syn_hip.h syn_edit: in-painting operands of syn_denoise_step_edit, token-major like x_t."""
    _fields_ = [("keep", vp), ("known", vp)]


class SynPlmsRow(C.Structure):
    """include/syn_hip.h syn_plms_row: one launch of a PLMS loop as syn_plms_update reads it from its device table."""
    _fields_ = [("r", C.c_float), ("inv_m", C.c_float), ("h_x", C.c_float), ("w_new", C.c_float), ("w", C.c_float * 3), ("store", i32)]


class SynBpdRow(C.Structure):
    """include/syn_hip.h syn_bpd_row: one timestep of the variational bound as syn_bpd_terms reads it from its device table."""
    _fields_ = [("c1", C.c_float), ("c2", C.c_float), ("log_var", C.c_float), ("r", C.c_float), ("inv_m", C.c_float), ("first", i32)]


SYN_OPT_MAX = 64
SYN_CONV_PACK_MAX = 40


class SynOptList(C.Structure):
    _fields_ = [("p", vp * SYN_OPT_MAX), ("g", vp * SYN_OPT_MAX), ("m", vp * SYN_OPT_MAX), ("v", vp * SYN_OPT_MAX),
                ("numel", i32 * SYN_OPT_MAX), ("n", i32)]


class SynConcatSrc(C.Structure):
    _fields_ = [("p", vp), ("p2", vp), ("width", i32), ("ld", i32), ("row_div", i32), ("pool", i32)]


class SynWgradSumJob(C.Structure):
    _fields_ = [("part", vp), ("dw", vp), ("n_clips", i32), ("l_out", i32), ("cin", i32), ("stride", i32), ("cout", i32), ("first_layer", i32),
                ("share_pitch", i32), ("reserved", i32)]


class SynBnFinalizeJob(C.Structure):
    _fields_ = [("part", vp), ("chunks", i32), ("channels", i32), ("rows", i64), ("gamma", vp), ("beta", vp), ("eps", C.c_float), ("momentum", C.c_float),
                ("run_mean", vp), ("run_var", vp), ("conv_bias", vp), ("stats", vp), ("affine", vp)]


class SynConvPackReq(C.Structure):
    _fields_ = [("w", vp), ("out_hi", vp), ("out_lo", vp), ("cout", i32), ("cin", i32), ("stride", i32), ("transposed", i32)]


class SynWavConv(C.Structure):
    _fields_ = [("w", vp), ("bias", vp)]


class SynWavEnc(C.Structure):
    _fields_ = [("cin", i32), ("reserved", i32), ("w_first", vp), ("conv", SynWavConv * 11)]


class SynCondWeights(C.Structure):
    _fields_ = [("gt", vp), ("tw", vp), ("st", vp), ("c0", vp), ("vocab", i32), ("seed_dim", i32), ("style_dim", i32), ("reserved", i32)]


class SynVqConv(C.Structure):
    _fields_ = [("w_packed", vp), ("bias", vp), ("cin", i32), ("cout", i32), ("cout_valid", i32), ("taps", i32),
                ("stride", i32), ("dil", i32), ("pad", i32), ("up", i32), ("relu_in", i32), ("relu_out", i32)]


class SynVqTrainPackJob(C.Structure):
    """include/syn_hip.h syn_vq_train_pack: one packing job, read by the kernel from device memory."""
    _fields_ = [("w", vp), ("out", vp), ("cout", i32), ("cin", i32), ("taps", i32), ("cout_p", i32), ("cin_p", i32), ("kind", i32)]


class SynVqModel(C.Structure):
    _fields_ = [("pose_dim", i32), ("reserved", i32), ("enc", SynVqConv * 16), ("dec", SynVqConv * 17),
                ("codebooks", vp), ("codebooks_t", vp), ("code_sq", vp)]


SYN_TMR_LAYERS = 4
SYN_TMR_MAX_LEN = 254       # include/syn_hip.h: rows per sequence without the two distribution tokens
SYN_TMR_MAX_FEATS = 4096


class SynTmrLayer(C.Structure):
    _fields_ = [("w_qkv", vp), ("b_qkv", vp), ("w_out", vp), ("b_out", vp), ("ln1_g", vp), ("ln1_b", vp),
                ("w_fc1", vp), ("b_fc1", vp), ("w_fc2", vp), ("b_fc2", vp), ("ln2_g", vp), ("ln2_b", vp)]


class SynTmrModel(C.Structure):
    _fields_ = [("nfeats", i32), ("relu_in", i32), ("w_in", vp), ("b_in", vp), ("mu_token", vp), ("logvar_token", vp), ("pe", vp),
                ("layer", SynTmrLayer * SYN_TMR_LAYERS)]


SYN_TMR_MAX_SEQ = 65536
SYN_BERT_D, SYN_BERT_HEADS, SYN_BERT_FF, SYN_BERT_MAX_LAYERS = 768, 12, 3072, 12      # include/syn_hip.h


class SynBertLayer(C.Structure):
    _fields_ = SynTmrLayer._fields_


class SynBertModel(C.Structure):
    _fields_ = [("n_layers", i32), ("vocab", i32), ("n_pos", i32), ("reserved", i32), ("word", vp), ("pos", vp), ("emb_ln_g", vp), ("emb_ln_b", vp),
                ("layer", SynBertLayer * SYN_BERT_MAX_LAYERS)]


SYN_SKEL_LAYERS = 4
SYN_SKEL_MAX_C = 384        # include/syn_hip.h: channels of a layer
SYN_SKEL_POOL_MAX = 4


class SynSkelLayer(C.Structure):
    _fields_ = [("w", vp), ("chunk_off", vp), ("chunk_k", vp), ("bias", vp), ("gn_g", vp), ("gn_b", vp), ("pool_src", vp), ("pool_w", vp),
                ("cin", i32), ("cout", i32), ("out_width", i32), ("reserved", i32)]


class SynSkelModel(C.Structure):
    _fields_ = [("layer", SynSkelLayer * SYN_SKEL_LAYERS)]


SYN_T2M_POSE, SYN_T2M_MOVE, SYN_T2M_MOTION_H, SYN_T2M_TEXT_H, SYN_T2M_WORD, SYN_T2M_POS, SYN_T2M_EMB = 619, 512, 1024, 512, 300, 15, 512
SYN_T2M_MAX_SEQ, SYN_T2M_MAX_FRAMES = 65536, 1024       # include/syn_hip.h
SYN_T2M_MOTION, SYN_T2M_TEXT = 0, 1


class SynT2mGru(C.Structure):
    _fields_ = [("w_ih", vp), ("b_ih", vp), ("w_hh", vp * 2), ("b_hh", vp), ("hidden", vp)]


class SynT2mHead(C.Structure):
    _fields_ = [("w1", vp), ("b1", vp), ("ln_g", vp), ("ln_b", vp), ("w2", vp), ("b2", vp)]


class SynT2mModel(C.Structure):
    _fields_ = [("conv1_w", vp), ("conv1_b", vp), ("conv2_w", vp), ("conv2_b", vp), ("out_w", vp), ("out_b", vp),
                ("motion_in_w", vp), ("motion_in_b", vp), ("motion_gru", SynT2mGru), ("motion_head", SynT2mHead),
                ("pos_w", vp), ("pos_b", vp), ("text_in_w", vp), ("text_in_b", vp), ("text_gru", SynT2mGru), ("text_head", SynT2mHead)]


class SynHipError(RuntimeError):
    pass


# ---- the ctypes signatures, read from the prototypes of include/syn_hip.h (the header is the contract; nothing is bound by hand) ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p, "void": None}
_MIRRORS = {n.lower(): c for n, c in list(globals().items()) if isinstance(c, type) and issubclass(c, C.Structure)}    # "synvqmodel" -> SynVqModel
# struct pointers that stay c_void_p: callers pass a device address (the tables, the job array) or a cast ctypes array (the requests) there
_RAW_STRUCT_POINTERS = {("syn_plms_update", "table"), ("syn_bpd_terms", "table"), ("syn_pack_weights", "jobs_dev"), ("syn_conv1d_pack_split_many", "reqs")}


def prototypes(header_text):
    """{name: (restype, argtypes)} of every `<ret> syn_name(<params>);` in the header.  Scalars map by width, a pointer to a syn_* struct to
    POINTER(its mirror above), every other pointer to c_void_p; a type outside that raises SynHipError naming the function - nothing is ever
    left to ctypes' default (which passes a 64-bit count or pointer as a C int)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*([\w \t*]+?)\s*\b(syn_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        ret = " ".join(ret.split()).replace(" *", "*")
        if ret not in _RETURNS:
            raise SynHipError(f"include/syn_hip.h: {name} returns `{ret}`, which the ctypes binding cannot map")
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(?:const\s+)?([\w ]+?)\s*(\**)\s*(\w+)\s*", p)
            base, stars, pname = m.groups() if m else (p, "", "")
            if base.startswith("syn_") and (name, pname) not in _RAW_STRUCT_POINTERS:
                base = _MIRRORS.get(base.replace("_", ""))            # None: a struct without a mirror
            if stars == "*" and isinstance(base, type):
                argtypes.append(C.POINTER(base))
            elif stars and (base in _SCALARS or base in ("void", "uint8_t", "uint32_t", "long long") or (name, pname) in _RAW_STRUCT_POINTERS):
                argtypes.append(C.c_void_p)
            elif not stars and base in _SCALARS:
                argtypes.append(_SCALARS[base])
            else:
                raise SynHipError(f"include/syn_hip.h: {name} takes `{' '.join(p.split())}`, which the ctypes binding cannot map")
        out[name] = (_RETURNS[ret], argtypes)
    return out


with open(HEADER_PATH) as _f:
    PROTOTYPES = prototypes(_f.read())
EXPORTS = tuple(n for n in PROTOTYPES if not n.startswith("syn_debug_"))
DIAGNOSTICS = tuple(n for n in PROTOTYPES if n.startswith("syn_debug_"))      # the process-wide `void syn_debug_*` switches (A/B runs and scripts/ only)

_lib = None


def load():
    """Load the shared library (once).  Raises SynHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SynHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback for the denoising path.")
    lib = C.CDLL(LIB_PATH)

    def bind(name):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = PROTOTYPES[name]
        return fn

    if bind("syn_version")() != ABI_VERSION:
        raise SynHipError(f"{LIB_PATH} has ABI version {lib.syn_version()}, this package needs {ABI_VERSION}: rebuild it "
                          "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name in PROTOTYPES:
        bind(name)
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().syn_last_error()
        raise SynHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream(device=None):
    """Raw hipStream_t of torch's current stream on `device` (a tensor's device; default: the current device).
    The library launches on the CURRENT HIP device (kernel attributes, device queries): a tensor that lives on another GPU than
    the one the calling thread has selected is refused here instead of being launched onto a stream that is not current."""
    import torch
    if device is not None:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
            raise SynHipError(f"tensors on {dev} but the current device is cuda:{torch.cuda.current_device()}: select the device first "
                              "(torch.cuda.set_device / `with torch.cuda.device(...)`, as nn.DataParallel and DDP do)")
    return torch.cuda.current_stream(device).cuda_stream
