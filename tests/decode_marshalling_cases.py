"""The boundary between the twelve public ops of a generation step and the C ABI, as data: a fixed list of calls on small CUDA
tensors, made with ``ops.call`` replaced by a recorder that forwards nothing -- no kernel is launched -- and per call the entry
point's name and its argument list, normalised so that no address is in it.  ``tools/record_decode_marshalling.py`` writes the list
to ``tests/golden/decode_marshalling.json``; ``tests/test_gpu_decode_marshalling.py`` makes the same calls and compares.  Public
names only: the same file runs at any commit whose ops have today's signatures.  Where a call under a forced plan of two key
ranges brings no workspace, the wrapper hands out its own grow-only buffer: the list then holds "other" for the address and "at least
N" for the size, N being the plan's bytes -- the buffer's real size depends on what the process ran before.

The calls are every STEP-th element of the product of the options below (heads 4, kv_heads 2, head_dim 128); ``_spread`` refuses a
step that leaves a value of an option out, so every value occurs for every op."""
import itertools

import torch

from mquant_amd import ops
from mquant_amd.ops import TiledAct

H, HKV, D = 4, 2, 128
QKV = (H + 2 * HKV) * D
E4M3 = torch.float8_e4m3fn
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
SHAPES = ((1, 1), (1, 64), (3, 64))                     # (R, capacity)
FORCE = (2, 32)                                         # two key ranges: for a call that brings its own workspace, or takes the wrapper's
POINTER = 1 << 32                                       # no count, stride or size in the list gets this far; every address does


def _spread(step, **options):
    """Every step-th combination of the options, as dicts; every value of every option must be among them."""
    names = list(options)
    picked = [dict(zip(names, c)) for c in itertools.product(*options.values())][::step]
    for n in names:
        assert {id(v) for v in options[n]} == {id(p[n]) for p in picked}, f"step {step} leaves a value of {n} out"
    return picked


class Recorder:
    """Stands in for ``ops.call``: keeps (entry point, normalised arguments) and launches nothing.  The one call it lets through is
    ``mq_attn_decode_debug_force``, which only sets two integers of the host's plan."""

    def __init__(self):
        self.real, self.names, self.last = ops.call, {}, None

    def __call__(self, name, *args):
        if name == "mq_attn_decode_debug_force":
            return self.real(name, *args)
        assert self.last is None, "one entry point per public call"
        self.last = (name, [self._norm(a) for a in args[:-1]] + ["stream"])

    def _norm(self, a):
        if a is None or isinstance(a, float):
            return a
        assert isinstance(a, int), type(a)
        return self.names.get(a, "other" if a >= POINTER else a)

    def run(self, fn, **kw):
        """fn(**kw) -> (entry point, arguments): the address of every tensor among kw becomes its keyword."""
        self.names = {v.data_ptr(): k for k, v in kw.items() if isinstance(v, (torch.Tensor, TiledAct))}
        assert len(self.names) == sum(isinstance(v, (torch.Tensor, TiledAct)) for v in kw.values()) and all(p >= POINTER for p in self.names)
        self.last = None
        fn(**kw)
        assert self.last is not None, "the call reached no entry point"
        return self.last


def _zeros(dev, dtype, *shape):
    nbytes = torch.empty((), dtype=dtype).element_size()
    return torch.zeros(shape[:-1] + (shape[-1] * nbytes,), dtype=torch.uint8, device=dev).view(dtype)


def _rows(dev, dtype, rows, width, strided, pad=128):
    """[rows, width]: contiguous, or the first columns of a buffer ``pad`` elements wider"""
    return _zeros(dev, dtype, rows, width + pad)[:, :width] if strided else _zeros(dev, dtype, rows, width)


def _cache(dev, storage, B, cap, layout):
    """[B, cap, 2 HKV, D] (B = None: one sequence's [cap, 2 HKV, D]): contiguous, rows 256 elements apart more, or -- batched --
    every sequence three rows longer than its capacity"""
    lead = () if B is None else (B,)
    if layout == "rows":
        return _zeros(dev, storage, *lead, cap, 2 * HKV * D + 256)[..., :2 * HKV * D].view(*lead, cap, 2 * HKV, D)
    if layout == "seq":
        return _zeros(dev, storage, B, cap + 3, 2 * HKV, D)[:, :cap]
    return _zeros(dev, storage, *lead, cap, 2 * HKV, D)


def _int32(dev, values):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _n_keys(dev, kind, B, R, cap):
    if kind == "int":
        return max(R, cap - 24) if cap > 1 else 1
    return None if kind is None else _int32(dev, [max(R, cap - 24 - b) if cap > 1 else 1 for b in range(B or 1)])


def _decode_calls(dev, scale):
    """(label, public op, keywords, forced plan or None) of the six attention ops"""
    I8 = torch.int8
    for batched, quant, fp8 in itertools.product((False, True), (False, True), (True, False)):
        if quant:
            fn = ops.attn_decode_quant_i8_batch if batched else ops.attn_decode_quant_i8
        elif fp8:
            fn = ops.attn_decode_fp8kv_batch if batched else ops.attn_decode_fp8kv
        else:
            fn = ops.attn_decode_batch if batched else ops.attn_decode
        options = dict(dt=list(DTYPES), shape=SHAPES, q=("packed", "strided"), cache=("packed", "rows") + (("seq",) if batched else ()),
                       n_keys=(None, "dev") + (() if batched else ("int",)), out=(None, "strided"), workspace=(None, "own", "the wrapper's"))
        if batched:
            options["B"] = (1, 3)
        if quant:
            options.update(tiled=(False, True), row_sel=(None, "mask"))
        for o in _spread({(False, False): 11, (False, True): 37, (True, False): 23, (True, True): 77}[batched, quant], **options):
            dt, (R, cap), B = DTYPES[o["dt"]], o["shape"], o.get("B")
            rows = (B or 1) * R
            q = _rows(dev, dt, rows, H * D, o["q"] == "strided", pad=QKV - H * D).view(*((B, R) if batched else (R,)), H, D)
            kw = dict(q=q, kv_cache=_cache(dev, E4M3 if fp8 else dt, B, cap, o["cache"]), n_keys=_n_keys(dev, o["n_keys"], B, R, cap),
                      causal=R > 1, out=None)
            if fp8 or quant:
                kw["kv_scale"] = scale if fp8 else None
            if quant:
                kw.update(scale0=0.25, scale1=0.5 if o["row_sel"] else None, tiled=o["tiled"],
                          row_sel=torch.ones((rows,), dtype=torch.uint8, device=dev) if o["row_sel"] else None)
                if o["out"]:
                    kw["out"] = TiledAct.empty(rows, H * D, dev) if o["tiled"] else _rows(dev, I8, rows, H * D, True)
            elif o["out"]:
                kw["out"] = _rows(dev, dt, rows, H * D, True)
            if o["workspace"] == "own":
                kw["workspace"] = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
            else:
                kw["softmax_scale"] = 0.125
            need = None
            if o["workspace"] == "the wrapper's":       # two ranges and no workspace given: the wrapper's grow-only buffer, of at least the plan's bytes
                T = kw["n_keys"] if isinstance(kw["n_keys"], int) else cap
                need = (lambda B=B, R=R, T=T: ops.attn_decode_batch_workspace_bytes(B, R, T, H, HKV) if B else ops.attn_decode_workspace_bytes(R, T, H, HKV))
            yield f"{fn.__name__} {'fp8' if fp8 else 'kv16'} {o}", fn, kw, FORCE if o["workspace"] else None, need


def _append_calls(dev, scale):
    for batched, fp8 in itertools.product((False, True), (True, False)):
        if fp8:
            fn = ops.kv_append_rope_fp8_batch if batched else ops.kv_append_rope_fp8
        else:
            fn = ops.kv_append_rope_batch if batched else ops.kv_append_rope
        options = dict(dt=list(DTYPES), shape=SHAPES, qkv=("packed", "strided"), cache=("packed", "rows") + (("seq",) if batched else ()),
                       n_keys=(None, "dev") + (() if batched else ("int",)), rope_delta=(None, "dev") + (() if batched else (0, 5)),
                       rope=(True, False))
        if batched:
            options["B"] = (1, 3)
        for o in _spread(19, **options):
            dt, (R, cap), B = DTYPES[o["dt"]], o["shape"], o.get("B")
            delta = _int32(dev, [3 + b for b in range(B or 1)]) if o["rope_delta"] == "dev" else o["rope_delta"]
            kw = dict(qkv=_rows(dev, dt, (B or 1) * R, QKV, o["qkv"] == "strided"), heads=H, kv_cache=_cache(dev, E4M3 if fp8 else dt, B, cap, o["cache"]),
                      n_keys=_n_keys(dev, o["n_keys"], B, R, cap), rope_delta=delta)
            if fp8:
                kw["kv_scale"] = scale
            if o["rope"]:
                kw.update(cos=_zeros(dev, dt, 96, D), sin=_zeros(dev, dt, 96, D))
            yield f"{fn.__name__} {o}", fn, kw, None, None


def _gather_calls(dev):
    for batched in (False, True):
        fn = ops.embed_gather_batch if batched else ops.embed_gather
        options = dict(dt=list(DTYPES), rows=(1, 3), table=("packed", "strided", "one row"), out=(None, "strided"),
                       id_log=(None, "packed") + (("rows",) if batched else ()), log_rows=(1, 64), n_keys=(None, "dev"))
        for o in _spread(7, **options):
            dt, rows, dim = DTYPES[o["dt"]], o["rows"], 64
            log_rows = max(o["log_rows"], 1 if batched else rows)
            kw = dict(table=_rows(dev, dt, 1 if o["table"] == "one row" else 16, dim, o["table"] != "packed"), ids=_int32(dev, list(range(rows))),
                      out=_rows(dev, dt, rows, dim, True) if o["out"] else None, id_log=None,
                      n_keys=_int32(dev, [log_rows] * (rows if batched else 1)) if o["n_keys"] else None)
            if o["id_log"]:
                kw["id_log"] = _rows(dev, torch.int32, rows, log_rows, o["id_log"] == "rows", pad=8) if batched else _int32(dev, [0] * log_rows)
            yield f"{fn.__name__} {o}", fn, kw, None, None


def record(dev="cuda:0"):
    """The list of {"call", "entry", "args"}: what the fixture holds."""
    dev = torch.device(dev)
    scale = torch.full((2 * HKV,), 0.5, dtype=torch.float32, device=dev)
    rec, out = Recorder(), []
    ops.call = rec
    try:
        for label, fn, kw, force, need in itertools.chain(_decode_calls(dev, scale), _append_calls(dev, scale), _gather_calls(dev)):
            if force:
                ops.attn_decode_debug_force(*force)
            try:
                entry, args = rec.run(fn, **kw)
                if need is not None and need():         # (workspace, workspace_bytes, stream) end every attention entry point's list
                    assert args[-3] == "other" and args[-2] >= need(), (label, args[-3:])
                    args[-2] = f"at least {need()}"
            finally:
                if force:
                    ops.attn_decode_debug_force(0, 0)
            out.append({"call": label, "entry": entry, "args": args})
    finally:
        ops.call = rec.real
    return out
