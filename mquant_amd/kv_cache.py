"""A KV cache whose length lives on the device: the state a captured generation step needs.

Per layer one cache ``[capacity, 2 * kv_heads, head_dim]`` (K heads then V heads), and for all layers ONE int32 ``n_keys`` on the
device -- the number of cache rows that hold keys -- plus an optional int32 ``rope_delta`` (HF Qwen2-VL's ``rope_deltas``: after an
image the text position is not the cache index).  A generation step is

    cache.advance(R)                       # n_keys += R, on the device, once per step
    for every layer:  qkv = <q|k|v projection of the R new rows>;  o = cache.step(layer, qkv, heads, out=...)

where ``step`` is two native calls that both read ``n_keys`` themselves: an append (rotate Q and K, write K|V into rows [n - R, n))
and a decode attention.  The cache keeps NO host copy of the length: after one warm-up step (the decode workspace and the one-time
check of the scales happen there) ``advance`` and ``step`` with ``out`` given neither synchronise nor allocate, so the step is
captured once into a graph and replayed while the cache grows.

ONE class, ``_DeviceLengthCache``, holds all of this.  It has two parameters, and the four public classes are its four
constructors:

    storage   e4m3 with per-layer scales (``Fp8KVCache*``: what ``ops.kv_quant_fp8`` writes; ``ops.kv_append_rope_fp8*`` and
              ``ops.attn_decode_fp8kv*``), or the model's dtype without scales (``KVCache16*``, the reference's default
              ``--k_bits 16 --v_bits 16``: ``ops.kv_append_rope*`` and ``ops.attn_decode*``)
    batch     None: one sequence; B (``*Batch``): B sequences that step together, so that one pass over the weights serves B tokens --
              per layer one buffer ``[B, capacity, 2 * kv_heads, head_dim]``, ``n_keys`` and ``rope_delta`` int32 ``[B]`` (every sequence
              has its own image, hence its own offset), ``step`` over qkv ``[B * R, ...]`` (rows [b R, (b + 1) R) belong to sequence b)
              as ONE batched append and ONE batched attention (the ``*_batch`` ops)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops

_E4M3 = torch.float8_e4m3fn
# (e4m3 storage, batched) -> the append, the attention and the attention with the fused quantizer of a step
_STEP_OPS = {
    (True, False): (ops.kv_append_rope_fp8, ops.attn_decode_fp8kv, ops.attn_decode_quant_i8),
    (False, False): (ops.kv_append_rope, ops.attn_decode, ops.attn_decode_quant_i8),
    (True, True): (ops.kv_append_rope_fp8_batch, ops.attn_decode_fp8kv_batch, ops.attn_decode_quant_i8_batch),
    (False, True): (ops.kv_append_rope_batch, ops.attn_decode_batch, ops.attn_decode_quant_i8_batch),
}


class _DeviceLengthCache:
    """The cache: the geometry, the RoPE tables, the per-layer buffers, the device integers and the step over them."""

    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, rope_delta, storage: torch.dtype,
                 kv_scales: Optional[Sequence[torch.Tensor]] = None, batch: Optional[int] = None):
        """storage: float8_e4m3fn with kv_scales, or ``dtype`` (fp16 / bf16) without.  kv_scales: per layer a float32 [2 * kv_heads]
        tensor (K scales then V scales; a [layers, 2 * kv_heads] tensor works), shared by the sequences of a batch (the scales are
        calibrated per layer, not per request).  cos / sin: the RoPE tables [rows, head_dim] in ``dtype`` (contiguous), or both None
        for a model without rotation at this point.  rope_delta: the initial position offset (a batch: B of them); None = no offset
        tensor at all (``set_rope_delta`` makes one later).  batch: None = one sequence, B = B sequences (a leading dimension
        everywhere)."""
        device = torch.device(device)
        assert (cos is None) == (sin is None) and (batch is None or batch >= 1)
        self.layers, self.capacity, self.kv_heads, self.head_dim, self.dtype = layers, capacity, kv_heads, head_dim, dtype
        self._lead = () if batch is None else (batch,)
        if batch is not None:
            self.batch = batch
        fp8 = storage == _E4M3
        if fp8:
            assert len(kv_scales) == layers
            self.scales = [s.to(device=device, dtype=torch.float32).contiguous() for s in kv_scales]
            for s in self.scales:
                assert s.numel() == 2 * kv_heads
        else:
            assert kv_scales is None and storage == dtype and dtype in (torch.float16, torch.bfloat16)
        self._kv_scale = self.scales if fp8 else [None] * layers         # per layer: the scales, or None for a 16-bit cache
        self._append_op, self._attend, self._attend_quant_i8 = _STEP_OPS[fp8, batch is not None]
        if cos is not None:
            assert cos.shape == sin.shape and cos.dim() == 2 and cos.shape[1] == head_dim
            cos, sin = cos.to(device=device, dtype=dtype).contiguous(), sin.to(device=device, dtype=dtype).contiguous()
        self.cos, self.sin = cos, sin
        nbytes = torch.empty((), dtype=storage).element_size()
        self.caches = [torch.zeros(self._lead + (capacity, 2 * kv_heads, head_dim * nbytes), dtype=torch.uint8, device=device).view(storage)
                       for _ in range(layers)]
        self.n_keys = torch.zeros(self._lead or (1,), dtype=torch.int32, device=device)
        self.rope_delta = None
        if rope_delta is not None:
            self.set_rope_delta(rope_delta)

    # ---- host side: bookkeeping (not for a captured step) ----
    def _store(self, values, into: torch.Tensor) -> None:
        if not self._lead:
            into.fill_(int(values))
            return
        values = [int(v) for v in values]
        assert len(values) == self.batch, f"{len(values)} values for a batch of {self.batch} sequences"
        into.copy_(torch.tensor(values, dtype=torch.int32))

    def set_length(self, n) -> None:
        """The number of keys the cache holds: an int, for a batch B of them."""
        assert all(0 <= int(v) <= self.capacity for v in (n if self._lead else [n])), f"length {n} outside the capacity {self.capacity}"
        self._store(n, self.n_keys)

    def set_rope_delta(self, delta) -> None:
        """Set the position offset (a batch: the B offsets) from the host.  The tensor is made on the first call: make it before a
        step is captured."""
        if self.rope_delta is None:
            self.rope_delta = torch.zeros_like(self.n_keys)
        self._store(delta, self.rope_delta)

    def fill(self, layer: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write of one sequence (the batched classes: ``fill(layer, b, kv_cols)``): kv_cols [T, 2 * kv_heads, head_dim] (K
        already rotated; the K|V columns of the fused q|k|v output work in place) into rows [0, T) of the layer's cache -- quantised by
        ``ops.kv_quant_fp8``, or for a 16-bit cache a bit copy of kv_cols in ``dtype``.  The length is set by ``set_length``, once for
        all layers."""
        return self._fill(layer, self.caches[layer], kv_cols)

    def _fill(self, layer: int, cache: torch.Tensor, kv_cols: torch.Tensor) -> torch.Tensor:
        T = kv_cols.shape[0]
        assert T <= self.capacity and tuple(kv_cols.shape[1:]) == (2 * self.kv_heads, self.head_dim)
        rows = cache[:T]
        if self._kv_scale[layer] is not None:
            return ops.kv_quant_fp8(kv_cols, self._kv_scale[layer], out=rows)
        assert kv_cols.dtype == self.dtype
        rows.copy_(kv_cols)
        return rows

    # ---- the generation step: capturable ----
    def advance(self, R: int = 1) -> None:
        """n_keys += R on the device (every sequence's): once per step, before the layers."""
        self.n_keys.add_(int(R))

    def _append(self, layer: int, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        scale = self._kv_scale[layer]
        if scale is None:                                              # the 16-bit ops have no scale argument
            self._append_op(qkv, heads, self.caches[layer], self.cos, self.sin, n_keys=self.n_keys, rope_delta=self.rope_delta)
        else:
            self._append_op(qkv, heads, self.caches[layer], scale, self.cos, self.sin, n_keys=self.n_keys, rope_delta=self.rope_delta)
        # the Q columns as [R, heads, D], a batch: [B, R, heads, D] -- ONE view op (the append has checked qkv's shape and strides)
        rows, ld, D = qkv.shape[0], qkv.stride(0), self.head_dim
        if self._lead:
            R = rows // self.batch
            return qkv.as_strided((self.batch, R, heads, D), (R * ld, ld, D, 1))
        return qkv.as_strided((rows, heads, D), (ld, D, 1))

    def step(self, layer: int, qkv: torch.Tensor, heads: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """qkv [R, (heads + 2 * kv_heads) * head_dim] (a batch: [B * R, ...]), the raw projection of the R newest positions (of every
        sequence; ``advance(R)`` came first): rotated and appended in place, then attended over the first n_keys rows (each sequence's
        own) -> [R, heads * head_dim] (a batch: [B * R, ...])."""
        q = self._append(layer, qkv, heads)
        scale = self._kv_scale[layer]
        if scale is None:
            return self._attend(q, self.caches[layer], n_keys=self.n_keys, causal=causal, out=out)
        return self._attend(q, self.caches[layer], scale, n_keys=self.n_keys, causal=causal, out=out)

    def step_quant_i8(self, layer: int, qkv: torch.Tensor, heads: int, scale0: float, scale1: Optional[float] = None, *,
                      causal: bool = True, row_sel: Optional[torch.Tensor] = None, out=None, tiled: bool = False):
        """``step`` with the next Linear's static int8 quantizer fused into the attention's store (``ops.attn_decode_quant_i8``, a
        batch: ``ops.attn_decode_quant_i8_batch``)."""
        q = self._append(layer, qkv, heads)
        return self._attend_quant_i8(q, self.caches[layer], self._kv_scale[layer], scale0, scale1, n_keys=self.n_keys, causal=causal,
                                     row_sel=row_sel, out=out, tiled=tiled)


class Fp8KVCache(_DeviceLengthCache):
    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, kv_scales: Sequence[torch.Tensor],
                 cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], device, dtype: torch.dtype,
                 rope_delta: Optional[int] = None):
        """One sequence over e4m3 caches.  The arguments: ``_DeviceLengthCache``."""
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, rope_delta, _E4M3, kv_scales)


class KVCache16(_DeviceLengthCache):
    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, rope_delta: Optional[int] = None):
        """``Fp8KVCache`` without scales: the caches hold ``dtype`` (fp16 / bf16)."""
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, rope_delta, dtype)


class _FillOfABatch:
    def fill(self, layer: int, b: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write of sequence b: ``fill`` of the single-sequence classes into rows [0, T) of its cache."""
        return self._fill(layer, self.caches[layer][b], kv_cols)


class Fp8KVCacheBatch(_FillOfABatch, _DeviceLengthCache):
    def __init__(self, batch: int, layers: int, capacity: int, kv_heads: int, head_dim: int, kv_scales: Sequence[torch.Tensor],
                 cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], device, dtype: torch.dtype,
                 rope_delta: Optional[Sequence[int]] = None):
        """``Fp8KVCache`` for ``batch`` sequences; rope_delta: the B initial offsets, or None."""
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, rope_delta, _E4M3, kv_scales, batch)


class KVCache16Batch(_FillOfABatch, _DeviceLengthCache):
    def __init__(self, batch: int, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, rope_delta: Optional[Sequence[int]] = None):
        """``KVCache16`` for ``batch`` sequences."""
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, rope_delta, dtype, batch=batch)
