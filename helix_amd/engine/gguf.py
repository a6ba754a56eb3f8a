"""GGUF v3 reader/writer: model loading and memory estimation.

The reference estimates GPU memory from GGUF tensor metadata
(api/pkg/memory/estimate.go) and serves GGUF checkpoints through
llama.cpp containers; here GGUF is a first-class *input format* for the
native engine: we parse the header, map llama.cpp tensor names onto our
fused-projection layout (models/llama.py), un-permute the Q/K rope
reordering applied by llama.cpp's HF converter, and dequantize
F32/F16/BF16/Q8_0/Q4_0/Q4_K/Q5_K/Q6_K tensors straight into bf16 device
weights, so a Q4_K_M or Q5_K_M file loads dense, embeddings and
output.weight included.

Quantized *serving*: `load_gguf_weights(..., keep_quantized=True)` keeps
projections resident as the file's own blocks (a strided copy into the
plane layouts of ops/hip/gemm_wq.hip and ops/hip/gemm_kq.hip, no
re-encoding) and dequantizes them inside the GEMM:
  * a projection whose parts are all Q4_0 or all Q8_0 becomes a
    models/quant.py WQLinear;
  * a projection whose parts are each Q4_K or Q6_K becomes a KQLinear with
    one segment per part; the parts may differ in type (a Q4_K_M file's
    qkv_proj is Q4_K, Q4_K, Q6_K). It needs K % 256 == 0 and every part's
    N % 16 == 0;
  * a Mixtral layer's experts (merged `ffn_gate_exps` / `ffn_up_exps` /
    `ffn_down_exps`, or the older per-expert `ffn_gate.{e}` names) whose gate
    and up are the same one of Q4_0/Q8_0 and whose down is one of them
    become MoEMLP's quantised planes (ops/hip/moe_wq.hip). The merged
    layout is ggml's convention as documented; like the K-quant decoders it
    has not been checked against a file written by llama.cpp;
  * a layer's experts whose gate and up are the same one of Q4_K/Q6_K and
    whose down is one of them become MoEMLP's K-quant planes
    (ops/hip/moe_kq.hip), layer by layer: a Q4_K_M file's ffn_down_exps
    are Q6_K in the layers q4_k_m_uses_q6_k selects and Q4_K in the others.
    It needs the hidden and the expert intermediate size to be multiples
    of 256. A layer that mixes the two families (Q4_0 gate, Q6_K down)
    loads dense.
Qwen3 (`general.architecture` qwen3 / qwen3moe): the per-head QK-norm
weights `attn_q_norm` / `attn_k_norm` load as tensors, and Q/K rows are taken
as they are: llama.cpp's converter permutes Q/K only for the llama
architecture, Qwen uses neox (rotate-half) rope. A dense Qwen3 Q4_K_M file
keeps its projections resident like a Llama one; a qwen3moe file keeps
Q4_0/Q8_0 and Q4_K/Q6_K experts (what a Q4_K_M qwen3moe file holds)
resident; Q5_K experts are dequantized to bf16. `qwen2` files are
still un-permuted like llama ones (an open point, docs/PARITY.md).
Everything else, including any other mix of types (Q4_0 with Q8_0, a
K-quant part next to a legacy or float part) and Q5_K, is dequantized to
the model dtype as before. `write_gguf` accepts pre-quantized
`GGMLQuantized` tensors so `helix export-gguf --quant` (and the tests) can
produce such files.

The K-quant decoders follow ggml's block_q4_K / block_q5_K / block_q6_K and
dequantize_row_* as written down in docs/KERNELS.md; no file written by
llama.cpp has been read with them yet. Q2_K/Q3_K and the IQ types stay
estimation-only.
"""
from __future__ import annotations

import struct
from typing import Any, BinaryIO, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

GGUF_MAGIC = b"GGUF"

# -- metadata value types (gguf spec) ----------------------------------
_T_U8, _T_I8, _T_U16, _T_I16, _T_U32, _T_I32 = 0, 1, 2, 3, 4, 5
_T_F32, _T_BOOL, _T_STRING, _T_ARRAY, _T_U64, _T_I64, _T_F64 = \
    6, 7, 8, 9, 10, 11, 12
_SCALAR_FMT = {
    _T_U8: "<B", _T_I8: "<b", _T_U16: "<H", _T_I16: "<h",
    _T_U32: "<I", _T_I32: "<i", _T_F32: "<f", _T_U64: "<Q",
    _T_I64: "<q", _T_F64: "<d",
}

# -- ggml tensor types: id -> (name, elems/block, bytes/block) ---------
GGML_TYPES: Dict[int, Tuple[str, int, int]] = {
    0: ("F32", 1, 4),
    1: ("F16", 1, 2),
    2: ("Q4_0", 32, 18),
    3: ("Q4_1", 32, 20),
    6: ("Q5_0", 32, 22),
    7: ("Q5_1", 32, 24),
    8: ("Q8_0", 32, 34),
    9: ("Q8_1", 32, 36),
    10: ("Q2_K", 256, 84),
    11: ("Q3_K", 256, 110),
    12: ("Q4_K", 256, 144),
    13: ("Q5_K", 256, 176),
    14: ("Q6_K", 256, 210),
    15: ("Q8_K", 256, 292),
    24: ("I8", 1, 1),
    25: ("I16", 1, 2),
    26: ("I32", 1, 4),
    27: ("I64", 1, 8),
    28: ("F64", 1, 8),
    30: ("BF16", 1, 2),
}
_NAME_TO_GGML = {v[0]: k for k, v in GGML_TYPES.items()}

# ggml type name <-> ops weight-only format string
_WQ_FMT = {"Q4_0": "q4_0", "Q8_0": "q8_0"}
# ggml type name <-> ops K-quant format string (resident types only)
_KQ_FMT = {"Q4_K": "q4_k", "Q6_K": "q6_k"}


class GGMLQuantized(NamedTuple):
    """A tensor already in ggml block bytes, for write_gguf."""
    raw: bytes
    shape: Tuple[int, ...]   # torch order ([out, in])
    type_name: str           # key of GGML_TYPES by name, e.g. "Q4_0"


def q4_k_m_uses_q6_k(layer: int, n_layers: int) -> bool:
    """llama.cpp's Q4_K_M recipe: the layers whose attn_v and ffn_down are
    Q6_K instead of Q4_K (integer division, as in use_more_bits)."""
    return (layer < n_layers // 8 or layer >= 7 * n_layers // 8
            or (layer - n_layers // 8) % 3 == 2)


def quantize_ggml(w: torch.Tensor, type_name: str) -> GGMLQuantized:
    """Quantize a [N, K] weight with ggml's reference Q4_0/Q8_0 quantizer,
    or with ops.quantize_kq's plain Q4_K/Q6_K quantizer."""
    from helix_amd import ops
    if type_name in _KQ_FMT:
        fmt = _KQ_FMT[type_name]
        return GGMLQuantized(ops.pack_ggml_kq(ops.quantize_kq(w, fmt), fmt),
                             tuple(w.shape), type_name)
    fmt = _WQ_FMT[type_name]
    qs, d = ops.quantize_wq(w, fmt)
    return GGMLQuantized(ops.pack_ggml(qs, d, fmt), tuple(w.shape), type_name)


class GGUFTensorInfo(NamedTuple):
    name: str
    shape: Tuple[int, ...]   # torch order ([out, in]); gguf stores reversed
    ggml_type: int
    offset: int              # relative to the aligned data section

    @property
    def numel(self) -> int:
        n = 1
        for d in self.shape:
            n *= d
        return n

    @property
    def nbytes(self) -> int:
        _, blk, bsz = GGML_TYPES[self.ggml_type]
        return (self.numel // blk) * bsz

    @property
    def type_name(self) -> str:
        return GGML_TYPES[self.ggml_type][0]


def _read_str(f: BinaryIO) -> str:
    (n,) = struct.unpack("<Q", f.read(8))
    return f.read(n).decode("utf-8")


def _read_value(f: BinaryIO, vtype: int) -> Any:
    if vtype in _SCALAR_FMT:
        fmt = _SCALAR_FMT[vtype]
        (v,) = struct.unpack(fmt, f.read(struct.calcsize(fmt)))
        return v
    if vtype == _T_BOOL:
        return f.read(1) != b"\x00"
    if vtype == _T_STRING:
        return _read_str(f)
    if vtype == _T_ARRAY:
        (etype,) = struct.unpack("<I", f.read(4))
        (count,) = struct.unpack("<Q", f.read(8))
        return [_read_value(f, etype) for _ in range(count)]
    raise ValueError(f"unknown gguf metadata type {vtype}")


class GGUFFile:
    """Parsed GGUF container: metadata dict + tensor directory.

    Tensor data is read lazily per-tensor (mmap-free sequential reads),
    so estimation never touches the multi-GB payload.
    """

    def __init__(self, path: str):
        self.path = path
        self.metadata: Dict[str, Any] = {}
        self.tensors: Dict[str, GGUFTensorInfo] = {}
        with open(path, "rb") as f:
            if f.read(4) != GGUF_MAGIC:
                raise ValueError(f"{path}: not a GGUF file")
            (self.version,) = struct.unpack("<I", f.read(4))
            if self.version < 2:
                raise ValueError(f"GGUF v{self.version} unsupported (<2)")
            n_tensors, n_kv = struct.unpack("<QQ", f.read(16))
            for _ in range(n_kv):
                key = _read_str(f)
                (vtype,) = struct.unpack("<I", f.read(4))
                self.metadata[key] = _read_value(f, vtype)
            for _ in range(n_tensors):
                name = _read_str(f)
                (nd,) = struct.unpack("<I", f.read(4))
                dims = struct.unpack(f"<{nd}Q", f.read(8 * nd))
                gtype, = struct.unpack("<I", f.read(4))
                (off,) = struct.unpack("<Q", f.read(8))
                if gtype not in GGML_TYPES:
                    raise ValueError(f"{name}: unknown ggml type {gtype}")
                # gguf dims are fastest-first; torch shape is the reverse
                self.tensors[name] = GGUFTensorInfo(
                    name, tuple(reversed(dims)), gtype, off)
            align = int(self.metadata.get("general.alignment", 32))
            pos = f.tell()
            self.data_start = (pos + align - 1) // align * align

    # -- sizing ---------------------------------------------------------
    def tensor_bytes(self) -> int:
        return sum(t.nbytes for t in self.tensors.values())

    def arch(self) -> Optional[str]:
        return self.metadata.get("general.architecture")

    # -- data -----------------------------------------------------------
    def read_raw(self, name: str) -> bytes:
        info = self.tensors[name]
        with open(self.path, "rb") as f:
            f.seek(self.data_start + info.offset)
            return f.read(info.nbytes)

    def load_tensor(self, name: str) -> torch.Tensor:
        """Dequantize one tensor to a torch tensor (fp32/bf16 source
        dtype preserved; Q-types dequantized to fp32)."""
        info = self.tensors[name]
        raw = self.read_raw(name)
        t = _dequantize(raw, info)
        return t.reshape(info.shape)


def _dequantize(raw: bytes, info: GGUFTensorInfo) -> torch.Tensor:
    tname = info.type_name
    if tname == "F32":
        return torch.from_numpy(
            np.frombuffer(raw, dtype="<f4").copy())
    if tname == "F16":
        return torch.from_numpy(
            np.frombuffer(raw, dtype="<f2").copy()).float()
    if tname == "BF16":
        u16 = np.frombuffer(raw, dtype="<u2").copy()
        return torch.from_numpy(u16).view(torch.bfloat16)
    if tname == "Q8_0":
        # block = f16 scale d + 32 int8 q; x = d * q
        blk = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 34)
        d = blk[:, :2].copy().view("<f2").astype(np.float32)
        qs = blk[:, 2:].copy().view(np.int8).astype(np.float32)
        return torch.from_numpy((d * qs).reshape(-1))
    if tname == "Q4_0":
        # block = f16 scale d + 16 nibble bytes; elem j in low nibbles,
        # elem j+16 in high nibbles; x = d * (nib - 8)
        blk = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 18)
        d = blk[:, :2].copy().view("<f2").astype(np.float32)
        qs = blk[:, 2:]
        lo = (qs & 0x0F).astype(np.float32) - 8.0
        hi = (qs >> 4).astype(np.float32) - 8.0
        out = np.concatenate([lo, hi], axis=1) * d
        return torch.from_numpy(out.reshape(-1))
    if tname in ("Q4_K", "Q5_K"):
        # super-block of 256 = d, dmin (f16), scales[12] (eight 6-bit
        # scale/min pairs), [Q5_K: qh[32], the fifth bits], qs[128];
        # x = (d*sc_j) * q - dmin*m_j per 32-element sub-block j
        bsz = 144 if tname == "Q4_K" else 176
        blk = np.frombuffer(raw, dtype=np.uint8).reshape(-1, bsz)
        d = blk[:, 0:2].copy().view("<f2").astype(np.float32)       # [B, 1]
        dmin = blk[:, 2:4].copy().view("<f2").astype(np.float32)
        s = blk[:, 4:16]
        sc = np.concatenate(
            [s[:, 0:4] & 63, (s[:, 8:12] & 0xF) | ((s[:, 0:4] >> 6) << 4)], 1)
        m = np.concatenate(
            [s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], 1)
        qs = blk[:, bsz - 128:].reshape(-1, 4, 1, 32)
        # bytes 32c..32c+31: low nibbles are sub-block 2c, high 2c+1
        q = np.concatenate([qs & 0x0F, qs >> 4], axis=2).reshape(-1, 8, 32)
        if tname == "Q5_K":
            qh = blk[:, 16:48].reshape(-1, 1, 32)
            bit = (qh >> np.arange(8, dtype=np.uint8).reshape(1, 8, 1)) & 1
            q = q + (bit << 4)
        ds = (d * sc.astype(np.float32))[:, :, None]
        dm = (dmin * m.astype(np.float32))[:, :, None]
        out = ds * q.astype(np.float32) - dm
        return torch.from_numpy(out.reshape(-1))
    if tname == "Q6_K":
        # super-block of 256 = ql[128], qh[64], scales[16] (int8), d (f16);
        # element 128h + 32g + l: low 4 bits from ql[64h + 32(g&1) + l]
        # (low nibble for g < 2), high 2 from (qh[32h + l] >> 2g) & 3;
        # x = (d * scales[8h + 2g + l/16]) * (q - 32)
        blk = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 210)
        ql = blk[:, :128].reshape(-1, 2, 2, 32)
        low = np.concatenate([ql & 0x0F, ql >> 4], axis=2)          # h, g, l
        qh = blk[:, 128:192].reshape(-1, 2, 1, 32)
        sh = (2 * np.arange(4, dtype=np.uint8)).reshape(1, 1, 4, 1)
        high = (qh >> sh) & 3
        q = (low | (high << 4)).astype(np.int32) - 32
        sc = blk[:, 192:208].copy().view(np.int8).astype(np.float32)
        d = blk[:, 208:210].copy().view("<f2").astype(np.float32)
        ds = (d * sc).reshape(-1, 2, 4, 2, 1)
        out = ds * q.reshape(-1, 2, 4, 2, 16).astype(np.float32)
        return torch.from_numpy(out.reshape(-1))
    raise NotImplementedError(
        f"dequantize {tname}: only F32/F16/BF16/Q8_0/Q4_0/Q4_K/Q5_K/Q6_K "
        f"supported (estimation supports all types)")


# -- llama.cpp -> helix_amd name mapping -------------------------------

def map_gguf_name(name: str):
    """llama.cpp tensor name -> (our param name, fuse-role)."""
    fixed = {
        "token_embd.weight": ("embed_tokens.weight", None),
        "output_norm.weight": ("final_norm_w", None),
        "output.weight": ("lm_head.weight", None),
    }
    if name in fixed:
        return fixed[name]
    if name.startswith("blk."):
        parts = name.split(".")
        i = parts[1]
        rest = ".".join(parts[2:])
        m = {
            "attn_norm.weight": (f"layers.{i}.input_norm_w", None),
            "ffn_norm.weight": (f"layers.{i}.post_norm_w", None),
            "attn_q.weight": (f"layers.{i}.attn.qkv_proj.weight", "q"),
            "attn_k.weight": (f"layers.{i}.attn.qkv_proj.weight", "k"),
            "attn_v.weight": (f"layers.{i}.attn.qkv_proj.weight", "v"),
            "attn_output.weight": (f"layers.{i}.attn.o_proj.weight", None),
            "attn_q_norm.weight": (f"layers.{i}.attn.q_norm_w", None),
            "attn_k_norm.weight": (f"layers.{i}.attn.k_norm_w", None),
            "ffn_gate.weight": (f"layers.{i}.mlp.gate_up_proj.weight",
                                "gate"),
            "ffn_up.weight": (f"layers.{i}.mlp.gate_up_proj.weight", "up"),
            "ffn_down.weight": (f"layers.{i}.mlp.down_proj.weight", None),
        }
        if rest in m:
            return m[rest]
        # Mixtral experts: the router, the merged [E, rows, K] tensors and
        # the older one-tensor-per-expert names ("gate_exp:3" = expert 3)
        moe = {
            "ffn_gate_inp.weight": (f"layers.{i}.mlp.router_w", None),
            "ffn_gate_exps.weight": (f"layers.{i}.mlp.w13", "gate_exps"),
            "ffn_up_exps.weight": (f"layers.{i}.mlp.w13", "up_exps"),
            "ffn_down_exps.weight": (f"layers.{i}.mlp.w2", "down_exps"),
        }
        if rest in moe:
            return moe[rest]
        if len(parts) == 5 and parts[4] == "weight" and parts[3].isdigit() \
                and parts[2] in _EXPERT_PARTS:
            role, attr = _EXPERT_PARTS[parts[2]]
            return f"layers.{i}.mlp.{attr}", f"{role}:{parts[3]}"
    return name, None


# per-expert legacy tensor `blk.i.<part>.<e>.weight` -> (role, MoEMLP attr)
_EXPERT_PARTS = {"ffn_gate": ("gate_exp", "w13"), "ffn_up": ("up_exp", "w13"),
                 "ffn_down": ("down_exp", "w2")}


def unpermute_rope(w: torch.Tensor, n_head: int) -> torch.Tensor:
    """Invert the Q/K row permutation llama.cpp's HF converter applies.

    The converter reorders each head's rows (n_head, 2, dh/2, in) ->
    swapaxes(1,2) so GGML's interleaved rope matches HF's half-rotation.
    Our rope is HF half-rotation (ops/hip/rope.hip), so loading GGUF we
    apply the inverse: (n_head, dh/2, 2, in) -> swapaxes(1,2).
    """
    out, inp = w.shape
    dh = out // n_head
    return (w.reshape(n_head, dh // 2, 2, inp)
            .swapaxes(1, 2).reshape(out, inp))


# architectures whose Q/K rows llama.cpp's converter leaves in HF order
# (neox rope): nothing to un-permute on load, nothing to permute on export
_NEOX_ARCHS = ("qwen3", "qwen3moe")


def _rows_permuted(arch: Optional[str]) -> bool:
    return (arch or "llama") not in _NEOX_ARCHS


# -- estimation (reference estimate.go role) ---------------------------

def estimate_gguf_bytes(path: str, kv_tokens: int = 0,
                        kv_dtype_bytes: int = 2) -> Dict[str, int]:
    """Memory footprint of serving a GGUF model: weights as stored
    (quantized sizes honored, like the reference's GGUF estimator) plus
    optional KV for `kv_tokens` cached tokens."""
    g = GGUFFile(path)
    weights = g.tensor_bytes()
    arch = g.arch() or "llama"
    n_layer = int(g.metadata.get(f"{arch}.block_count", 0))
    n_kv_head = int(g.metadata.get(
        f"{arch}.attention.head_count_kv",
        g.metadata.get(f"{arch}.attention.head_count", 0)))
    n_embd = int(g.metadata.get(f"{arch}.embedding_length", 0))
    n_head = int(g.metadata.get(f"{arch}.attention.head_count", 1))
    # Qwen3's head_dim is not n_embd / n_head; such files say so
    head_dim = int(g.metadata.get(f"{arch}.attention.key_length",
                                  n_embd // max(1, n_head)))
    kv = 2 * n_layer * n_kv_head * head_dim * kv_tokens * kv_dtype_bytes
    return {"weights": weights, "kv": kv, "total": weights + kv}


# -- writer (tests + checkpoint export) --------------------------------

def _write_str(f: BinaryIO, s: str):
    b = s.encode("utf-8")
    f.write(struct.pack("<Q", len(b)))
    f.write(b)


def _write_value(f: BinaryIO, v: Any):
    if isinstance(v, bool):
        f.write(struct.pack("<I", _T_BOOL))
        f.write(b"\x01" if v else b"\x00")
    elif isinstance(v, int):
        f.write(struct.pack("<I", _T_U32 if 0 <= v < 2**32 else _T_I64))
        f.write(struct.pack("<I" if 0 <= v < 2**32 else "<q", v))
    elif isinstance(v, float):
        f.write(struct.pack("<I", _T_F32))
        f.write(struct.pack("<f", v))
    elif isinstance(v, str):
        f.write(struct.pack("<I", _T_STRING))
        _write_str(f, v)
    else:
        raise TypeError(f"unsupported metadata value {type(v)}")


def write_gguf(path: str, metadata: Dict[str, Any],
               tensors: Dict[str, Any], align: int = 32):
    """Write a GGUF v3 file. Values are torch tensors (F32/F16/BF16
    payloads) or GGMLQuantized (block bytes written as they are). Used by
    tests and `helix export-gguf`."""
    # (name, payload bytes, torch-order shape, ggml type, offset)
    infos: List[Tuple[str, bytes, Tuple[int, ...], int, int]] = []
    off = 0
    for name, t in tensors.items():
        if isinstance(t, GGMLQuantized):
            if t.type_name not in _NAME_TO_GGML:
                raise TypeError(f"{name}: unknown ggml type {t.type_name}")
            gt = _NAME_TO_GGML[t.type_name]
            _, blk, bsz = GGML_TYPES[gt]
            numel = 1
            for dim in t.shape:
                numel *= dim
            if not t.shape or t.shape[-1] % blk or \
                    len(t.raw) != numel // blk * bsz:
                raise ValueError(
                    f"{name}: {len(t.raw)} bytes do not match shape "
                    f"{tuple(t.shape)} of {t.type_name}")
            buf, shape = bytes(t.raw), tuple(t.shape)
        else:
            t = t.detach().cpu().contiguous()
            if t.dtype == torch.float32:
                gt = _NAME_TO_GGML["F32"]
            elif t.dtype == torch.float16:
                gt = _NAME_TO_GGML["F16"]
            elif t.dtype == torch.bfloat16:
                gt = _NAME_TO_GGML["BF16"]
            else:
                raise TypeError(f"{name}: dtype {t.dtype} not writable")
            if t.dtype == torch.bfloat16:
                buf = t.view(torch.uint16).numpy().tobytes()
            else:
                buf = t.numpy().tobytes()
            shape = tuple(t.shape)
        infos.append((name, buf, shape, gt, off))
        off += (len(buf) + align - 1) // align * align
    with open(path, "wb") as f:
        f.write(GGUF_MAGIC)
        f.write(struct.pack("<I", 3))
        meta = dict(metadata)
        meta.setdefault("general.alignment", align)
        f.write(struct.pack("<QQ", len(infos), len(meta)))
        for k, v in meta.items():
            _write_str(f, k)
            _write_value(f, v)
        for name, buf, shape, gt, o in infos:
            _write_str(f, name)
            dims = tuple(reversed(shape)) if shape else (1,)
            f.write(struct.pack("<I", len(dims)))
            f.write(struct.pack(f"<{len(dims)}Q", *dims))
            f.write(struct.pack("<I", gt))
            f.write(struct.pack("<Q", o))
        pos = f.tell()
        f.write(b"\x00" * ((pos + align - 1) // align * align - pos))
        for name, buf, shape, gt, o in infos:
            f.write(buf)
            pad = (len(buf) + align - 1) // align * align - len(buf)
            f.write(b"\x00" * pad)


# fused projection -> (GGUF part suffixes in row order, role per part)
_FUSED_PARTS = {
    "attn.qkv_proj": (("attn_q", "q"), ("attn_k", "k"), ("attn_v", "v")),
    "attn.o_proj": (("attn_output", None),),
    "mlp.gate_up_proj": (("ffn_gate", "gate"), ("ffn_up", "up")),
    "mlp.down_proj": (("ffn_down", None),),
}


def _install_resident(model, g: GGUFFile) -> set:
    """Install every projection whose GGUF parts are all the same one of
    Q4_0/Q8_0 as a WQLinear, and every projection whose parts are each
    Q4_K or Q6_K (not necessarily the same) as a KQLinear with one segment
    per part, holding the file's blocks. Any other mix stays dense.
    Returns the GGUF tensor names consumed."""
    from helix_amd import ops
    from helix_amd.models.quant import (KQLinear, WQLinear,
                                        attach_wq_scratch)
    cfg = model.cfg
    todo = []
    for i in range(cfg.num_layers):
        for proj, parts in _FUSED_PARTS.items():
            names = [f"blk.{i}.{p}.weight" for p, _ in parts]
            if not all(n in g.tensors for n in names):
                continue
            types = [g.tensors[n].type_name for n in names]
            if len(set(types)) == 1 and types[0] in _WQ_FMT:
                fmts, block = [_WQ_FMT[types[0]]] * len(names), 32
            elif all(t in _KQ_FMT for t in types):
                fmts, block = [_KQ_FMT[t] for t in types], 256
            else:
                continue
            owner = model.get_submodule(f"layers.{i}.{proj.split('.')[0]}")
            lin = getattr(owner, proj.split(".")[1])
            if not isinstance(lin, torch.nn.Linear):
                continue
            infos = [g.tensors[n] for n in names]
            if any(len(t.shape) != 2 or t.shape[1] != lin.in_features
                   for t in infos) or \
                    sum(t.shape[0] for t in infos) != lin.out_features or \
                    lin.in_features % block or lin.out_features % 16:
                continue
            # a K-quant segment is a launch of its own: each part's rows
            # must be whole 16-channel tiles
            if block == 256 and any(t.shape[0] % 16 for t in infos):
                continue
            todo.append((owner, proj.split(".")[1], lin, names, parts, fmts))
    if not todo:
        return set()
    dev = todo[0][2].weight.device
    used = set()
    permuted = _rows_permuted(g.arch())
    for owner, attr, lin, names, parts, fmts in todo:
        kq = fmts[0] in _KQ_FMT.values()
        plane_parts = []
        for n, (_, role), fmt in zip(names, parts, fmts):
            unpack = ops.unpack_ggml_kq if kq else ops.unpack_ggml
            planes = unpack(g.read_raw(n), g.tensors[n].shape, fmt)
            # a block never crosses a row, so the Q/K row permutation
            # applies to every plane as whole rows
            heads = {"q": cfg.num_heads, "k": cfg.num_kv_heads}.get(role)
            if heads is not None and permuted:
                planes = tuple(
                    unpermute_rope(p.reshape(p.shape[0], -1), heads)
                    .reshape(p.shape) for p in planes)
            plane_parts.append(planes)
            used.add(n)
        # the bias stays the model's own: map_gguf_name maps no bias tensor
        # today; when it does, the loader must write the module's bias,
        # which is a buffer and not among named_parameters()
        bias = None if lin.bias is None else lin.bias.data
        if kq:
            mod = KQLinear(
                [(fmt, tuple(p.contiguous().to(dev) for p in planes))
                 for fmt, planes in zip(fmts, plane_parts)], bias)
        else:
            qs, d = (torch.cat(ps, dim=0).contiguous().to(dev)
                     for ps in zip(*plane_parts))
            mod = WQLinear(qs, d, fmts[0], bias)
        setattr(owner, attr, mod)
    attach_wq_scratch(model)
    return used


def _expert_tensor_names(g: GGUFFile, i: int, E: int):
    """[gate names, up names, down names] of layer i's experts: one merged
    tensor each, or E per-expert tensors each (the older layout); None when
    the file has neither complete."""
    merged = [[f"blk.{i}.ffn_{p}_exps.weight"] for p in ("gate", "up", "down")]
    if all(n[0] in g.tensors for n in merged):
        return merged
    legacy = [[f"blk.{i}.ffn_{p}.{e}.weight" for e in range(E)]
              for p in ("gate", "up", "down")]
    if all(n in g.tensors for part in legacy for n in part):
        return legacy
    return None


def _install_resident_experts(model, g: GGUFFile) -> set:
    """Keep a layer's experts as the file's blocks (MoEMLP's quantised
    state) when gate and up are the same one of Q4_0/Q8_0 and down is one of
    Q4_0/Q8_0, or gate and up are the same one of Q4_K/Q6_K and down is one
    of Q4_K/Q6_K (MoEMLP's K-quant state; needs H and I to be multiples of
    256). The formats are per layer: a Q4_K_M file's ffn_down_exps are Q6_K
    in some layers and Q4_K in the others. Any other mix, one across the two
    families included, is left to the dense loader. Returns the GGUF tensor
    names consumed."""
    from helix_amd import ops
    from helix_amd.models.quant import attach_wq_scratch
    cfg = model.cfg
    E, H, I = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    used = set()
    if E == 0 or H % 32 or I % 32:
        return used
    for i in range(cfg.num_layers):
        mlp = model.get_submodule(f"layers.{i}.mlp")
        if getattr(mlp, "expert_fmt", True) is not None:
            continue                       # no MoEMLP, or already quantised
        names = _expert_tensor_names(g, i, E)
        if names is None:
            continue
        types = [{g.tensors[n].type_name for n in part} for part in names]
        if any(len(t) != 1 for t in types):
            continue
        tg, tu, td = (next(iter(t)) for t in types)
        if tg == tu and tg in _WQ_FMT and td in _WQ_FMT:
            family, unpack = _WQ_FMT, ops.unpack_ggml
        elif tg == tu and tg in _KQ_FMT and td in _KQ_FMT \
                and H % 256 == 0 and I % 256 == 0:
            family, unpack = _KQ_FMT, ops.unpack_ggml_kq
        else:
            continue
        shapes = [(I, H), (I, H), (H, I)]
        if any(tuple(g.tensors[n].shape) !=
               ((E,) + s if len(part) == 1 else s)
               for part, s in zip(names, shapes) for n in part):
            continue
        dev = mlp.router_w.device
        planes = []
        for part, (rows, K), t in zip(names, shapes, (tg, tu, td)):
            # rows are independent (a block or super-block never crosses a
            # row): a merged tensor is [E*rows, K]
            n_rows = E * rows if len(part) == 1 else rows
            got = [unpack(g.read_raw(n), (n_rows, K), family[t])
                   for n in part]
            planes.append(tuple(
                torch.cat(ps, dim=0).view(E, rows, *ps[0].shape[1:])
                for ps in zip(*got)))
            used.update(part)
        gate, up, down = planes
        w13 = tuple(torch.cat([a, b], dim=1).contiguous().to(dev)
                    for a, b in zip(gate, up))
        w2 = tuple(p.contiguous().to(dev) for p in down)
        if family is _KQ_FMT:
            mlp.set_kquant_experts(w13, w2, (family[tg], family[td]))
        else:
            mlp.set_quantized_experts(w13, w2, (family[tg], family[td]))
    if used:
        attach_wq_scratch(model)
    return used


def _check_expert_metadata(cfg, g: GGUFFile) -> None:
    arch = g.arch() or "llama"
    for key, want in ((f"{arch}.expert_count", cfg.num_experts),
                      (f"{arch}.expert_used_count", cfg.experts_per_token)):
        if key in g.metadata and int(g.metadata[key]) != \
                (want if cfg.num_experts > 0 else 0):
            raise ValueError(
                f"{g.path}: {key} = {g.metadata[key]}, but preset "
                f"{cfg.name!r} has {want if cfg.num_experts > 0 else 0}")


@torch.inference_mode()
def load_gguf_weights(model, path: str, keep_quantized: bool = False) -> int:
    """Load a GGUF llama checkpoint into a helix_amd Llama model
    (dequantizing to the model dtype; Q/K rope rows un-permuted, except
    for the qwen3 / qwen3moe architectures, whose rows are not permuted in
    the file). With
    keep_quantized, Q4_0/Q8_0 projections (WQLinear), Q4_K/Q6_K
    projections (KQLinear) and Q4_0/Q8_0 or Q4_K/Q6_K experts (MoEMLP's
    planes) stay resident as the file's blocks; see the module docstring.
    A file whose
    expert_count / expert_used_count differ from the model's is refused."""
    g = GGUFFile(path)
    _check_expert_metadata(model.cfg, g)
    resident = _install_resident(model, g) if keep_quantized else set()
    if keep_quantized:
        resident |= _install_resident_experts(model, g)
    params = dict(model.named_parameters())
    cfg = model.cfg
    q, kv = cfg.q_size, cfg.kv_size
    inter = cfg.intermediate_size
    loaded = len(resident)
    permuted = _rows_permuted(g.arch())
    for name in g.tensors:
        if name in resident:
            continue
        our, role = map_gguf_name(name)
        if our not in params:
            continue
        t = g.load_tensor(name)
        if role == "q" and permuted:
            t = unpermute_rope(t, cfg.num_heads)
        elif role == "k" and permuted:
            t = unpermute_rope(t, cfg.num_kv_heads)
        p = params[our]
        t = t.to(p.dtype)
        if role == "q":
            p.data[:q].copy_(t)
        elif role == "k":
            p.data[q:q + kv].copy_(t)
        elif role == "v":
            p.data[q + kv:].copy_(t)
        elif role == "gate":
            p.data[:inter].copy_(t)
        elif role == "up":
            p.data[inter:].copy_(t)
        elif role == "gate_exps":               # merged [E, I, H]
            p.data[:, :inter].copy_(t)
        elif role == "up_exps":
            p.data[:, inter:].copy_(t)
        elif role is not None and ":" in role:  # one expert's tensor
            kind, e = role.split(":")
            if kind == "gate_exp":
                p.data[int(e), :inter].copy_(t)
            elif kind == "up_exp":
                p.data[int(e), inter:].copy_(t)
            else:
                p.data[int(e)].copy_(t)
        else:
            p.data.copy_(t)
        loaded += 1
    return loaded


# -- export (`helix export-gguf`) ---------------------------------------

EXPORT_QUANTS = ("", "q4_0", "q8_0", "q4_k", "q6_k", "q4_k_m")


EXPORT_EXPERT_QUANTS = ("q4_k", "q6_k", "q4_k_m")


def export_model_gguf(model, path: str, quant: str = "",
                      experts_only: bool = False,
                      expert_quant: Optional[str] = None) -> int:
    """Write `model` (a dense LlamaForCausalLM, experts in bf16 if it has
    any) as a GGUF v3 checkpoint with llama.cpp tensor names, Q/K rows
    permuted for GGML rope. `quant` quantizes the projection weights (norms
    and embeddings stay as they are) as `helix export-gguf --quant` says.
    A mixture of experts writes the router, the merged ffn_*_exps tensors
    ([E, rows, K]) and llama.expert_count / expert_used_count; q4_0 / q8_0
    quantize the experts too (quantize_ggml on the flattened rows), the
    K-quant flags leave them bf16. experts_only: quantize nothing but the
    experts. expert_quant ("q4_k" / "q6_k" / "q4_k_m", a mixture of experts
    only, not next to quant q4_0 / q8_0) writes the experts as K-quant
    super-blocks whatever `quant` does to the rest: q4_k_m is Q4_K gate and
    up, and Q6_K down in the layers q4_k_m_uses_q6_k selects, Q4_K in the
    others; it needs the experts' K to be a multiple of 256. A model with QK-norm (Qwen3) is written as architecture
    qwen3 / qwen3moe: its `{arch}.*` keys, attention.key_length /
    value_length, the attn_q_norm / attn_k_norm tensors, and Q/K rows as
    they are (no permutation). Returns the number of tensors written."""
    if quant not in EXPORT_QUANTS:
        raise ValueError(f"quant must be one of {EXPORT_QUANTS[1:]}")
    cfg = model.cfg
    if expert_quant is not None:
        if expert_quant not in EXPORT_EXPERT_QUANTS:
            raise ValueError(
                f"expert_quant must be one of {EXPORT_EXPERT_QUANTS}")
        if cfg.num_experts == 0:
            raise ValueError("expert_quant: the model has no experts")
        if quant in ("q4_0", "q8_0"):
            raise ValueError(f"expert_quant: quant={quant!r} already "
                             "quantises the experts")
        if cfg.hidden_size % 256 or cfg.intermediate_size % 256:
            raise ValueError("expert_quant: hidden and intermediate sizes "
                             "must be multiples of 256")

    moe = cfg.num_experts > 0
    qk_norm = getattr(cfg, "qk_norm", False)
    arch = ("qwen3moe" if moe else "qwen3") if qk_norm else "llama"

    def permute(w, n_head):
        if not _rows_permuted(arch):
            return w
        o, i = w.shape
        return (w.reshape(n_head, 2, o // n_head // 2, i)
                .swapaxes(1, 2).reshape(o, i))

    sd = dict(model.named_parameters())
    q, kv, inter = cfg.q_size, cfg.kv_size, cfg.intermediate_size
    tensors = {
        "token_embd.weight": sd["embed_tokens.weight"].data,
        "output_norm.weight": sd["final_norm_w"].data,
        "output.weight": sd["lm_head.weight"].data,
    }
    for i in range(cfg.num_layers):
        qkv = sd[f"layers.{i}.attn.qkv_proj.weight"].data
        tensors[f"blk.{i}.attn_q.weight"] = permute(qkv[:q], cfg.num_heads)
        tensors[f"blk.{i}.attn_k.weight"] = permute(qkv[q:q + kv],
                                                    cfg.num_kv_heads)
        tensors[f"blk.{i}.attn_v.weight"] = qkv[q + kv:]
        tensors[f"blk.{i}.attn_output.weight"] = \
            sd[f"layers.{i}.attn.o_proj.weight"].data
        if qk_norm:
            tensors[f"blk.{i}.attn_q_norm.weight"] = \
                sd[f"layers.{i}.attn.q_norm_w"].data
            tensors[f"blk.{i}.attn_k_norm.weight"] = \
                sd[f"layers.{i}.attn.k_norm_w"].data
        if moe:
            if f"layers.{i}.mlp.w13" not in sd:
                raise ValueError("export_model_gguf: the experts of layer "
                                 f"{i} are already quantised")
            w13 = sd[f"layers.{i}.mlp.w13"].data
            tensors[f"blk.{i}.ffn_gate_inp.weight"] = \
                sd[f"layers.{i}.mlp.router_w"].data
            tensors[f"blk.{i}.ffn_gate_exps.weight"] = w13[:, :inter]
            tensors[f"blk.{i}.ffn_up_exps.weight"] = w13[:, inter:]
            tensors[f"blk.{i}.ffn_down_exps.weight"] = \
                sd[f"layers.{i}.mlp.w2"].data
        else:
            gu = sd[f"layers.{i}.mlp.gate_up_proj.weight"].data
            tensors[f"blk.{i}.ffn_gate.weight"] = gu[:inter]
            tensors[f"blk.{i}.ffn_up.weight"] = gu[inter:]
            tensors[f"blk.{i}.ffn_down.weight"] = \
                sd[f"layers.{i}.mlp.down_proj.weight"].data
        tensors[f"blk.{i}.attn_norm.weight"] = \
            sd[f"layers.{i}.input_norm_w"].data
        tensors[f"blk.{i}.ffn_norm.weight"] = \
            sd[f"layers.{i}.post_norm_w"].data
    meta = {
        "general.architecture": arch,
        "general.name": cfg.name,
        f"{arch}.block_count": cfg.num_layers,
        f"{arch}.embedding_length": cfg.hidden_size,
        f"{arch}.feed_forward_length": cfg.intermediate_size,
        f"{arch}.attention.head_count": cfg.num_heads,
        f"{arch}.attention.head_count_kv": cfg.num_kv_heads,
        f"{arch}.context_length": cfg.max_position,
        f"{arch}.rope.freq_base": float(cfg.rope_base),
    }
    if qk_norm:
        meta[f"{arch}.attention.key_length"] = cfg.head_dim
        meta[f"{arch}.attention.value_length"] = cfg.head_dim
        meta[f"{arch}.attention.layer_norm_rms_epsilon"] = \
            float(cfg.rms_norm_eps)
        if moe:
            meta[f"{arch}.expert_feed_forward_length"] = \
                cfg.intermediate_size
    if moe:
        meta[f"{arch}.expert_count"] = cfg.num_experts
        meta[f"{arch}.expert_used_count"] = cfg.experts_per_token
    if quant:
        proj = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate",
                "ffn_up", "ffn_down")
        exps = ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps")
        block = 256 if quant.endswith(("_k", "_k_m")) else 32
        for name, t in list(tensors.items()):
            part = name.split(".")[2] if name.startswith("blk.") else ""
            if part in exps:
                # [E, rows, K]: rows are independent, so quantize the
                # flattened rows and keep the 3-D shape
                if block == 32 and t.shape[2] % 32 == 0:
                    qt = quantize_ggml(t.reshape(-1, t.shape[2]),
                                       quant.upper())
                    tensors[name] = GGMLQuantized(qt.raw, tuple(t.shape),
                                                  qt.type_name)
                continue
            if experts_only or part not in proj or t.shape[1] % block:
                continue
            gtype = quant.upper()
            if quant == "q4_k_m":
                # llama.cpp's recipe: Q4_K, with Q6_K for attn_v and
                # ffn_down in the layers q4_k_m_uses_q6_k selects
                layer = int(name.split(".")[1])
                more = part in ("attn_v", "ffn_down") and \
                    q4_k_m_uses_q6_k(layer, cfg.num_layers)
                gtype = "Q6_K" if more else "Q4_K"
            tensors[name] = quantize_ggml(t, gtype)
        if quant == "q4_k_m" and not experts_only:
            for name, gtype in (("output.weight", "Q6_K"),
                                ("token_embd.weight", "Q4_K")):
                if tensors[name].shape[1] % 256 == 0:
                    tensors[name] = quantize_ggml(tensors[name], gtype)
    if expert_quant is not None:
        for name, t in list(tensors.items()):
            part = name.split(".")[2] if name.startswith("blk.") else ""
            if not part.endswith("_exps"):
                continue
            gtype = "Q6_K" if expert_quant == "q6_k" else "Q4_K"
            if expert_quant == "q4_k_m" and part == "ffn_down_exps" and \
                    q4_k_m_uses_q6_k(int(name.split(".")[1]), cfg.num_layers):
                gtype = "Q6_K"
            qt = quantize_ggml(t.reshape(-1, t.shape[2]), gtype)
            tensors[name] = GGMLQuantized(qt.raw, tuple(t.shape),
                                          qt.type_name)
    write_gguf(path, meta, tensors)
    return len(tensors)
