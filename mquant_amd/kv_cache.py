"""An e4m3 KV cache whose length lives on the device: the state a captured generation step needs.

Per layer one cache ``[capacity, 2 * kv_heads, head_dim]`` (K heads then V heads, what ``ops.kv_quant_fp8`` writes), and for all
layers ONE int32 ``n_keys`` on the device -- the number of cache rows that hold keys -- plus an optional int32 ``rope_delta``
(HF Qwen2-VL's ``rope_deltas``: after an image the text position is not the cache index).  A generation step is

    cache.advance(R)                       # n_keys += R, on the device, once per step
    for every layer:  qkv = <q|k|v projection of the R new rows>;  o = cache.step(layer, qkv, heads, out=...)

where ``step`` is two native calls that both read ``n_keys`` themselves: ``ops.kv_append_rope_fp8`` (rotate Q and K, quantise K|V
into rows [n - R, n)) and ``ops.attn_decode_fp8kv``.  The class keeps NO host copy of the length: after one warm-up step (the
decode workspace and the one-time check of the scales happen there) ``advance`` and ``step`` with ``out`` given neither
synchronise nor allocate, so the step is captured once into a graph and replayed while the cache grows.

``KVCache16`` is the same object for the reference's default KV setting (``--k_bits 16 --v_bits 16``: K / V stay in the model's
dtype): the caches hold ``dtype`` instead of e4m3, there are no scales, and ``step`` is ``ops.kv_append_rope`` and
``ops.attn_decode``.  Same interface, same contract; what does not depend on the storage lives in one base class.

``Fp8KVCacheBatch`` and ``KVCache16Batch`` are the two classes for B sequences that step together, so that one pass over the weights
serves B tokens: per layer one buffer ``[B, capacity, 2 * kv_heads, head_dim]``, ``n_keys`` and ``rope_delta`` int32 ``[B]``, ``step`` over
qkv ``[B * R, ...]`` as ONE batched append and ONE batched attention (``ops.kv_append_rope*_batch``, ``ops.attn_decode*_batch``)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops


class _DeviceLengthCache:
    """What the two cache classes share: the geometry, the RoPE tables, the per-layer buffers and the two device integers."""

    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, storage: torch.dtype, rope_delta, batch: Optional[int] = None):
        """batch: None = one sequence (buffers [capacity, ...], one length); B = the batched classes below ([B, capacity, ...], B lengths)."""
        device = torch.device(device)
        assert (cos is None) == (sin is None)
        lead = () if batch is None else (batch,)
        self.layers, self.capacity, self.kv_heads, self.head_dim, self.dtype = layers, capacity, kv_heads, head_dim, dtype
        if cos is not None:
            assert cos.shape == sin.shape and cos.dim() == 2 and cos.shape[1] == head_dim
            cos, sin = cos.to(device=device, dtype=dtype).contiguous(), sin.to(device=device, dtype=dtype).contiguous()
        self.cos, self.sin = cos, sin
        nbytes = torch.empty((), dtype=storage).element_size()
        self.caches = [torch.zeros(lead + (capacity, 2 * kv_heads, head_dim * nbytes), dtype=torch.uint8, device=device).view(storage)
                       for _ in range(layers)]
        self.n_keys = torch.zeros(lead or (1,), dtype=torch.int32, device=device)
        self.rope_delta = None
        if rope_delta is not None:
            self.set_rope_delta(rope_delta)

    # ---- host side: bookkeeping (not for a captured step) ----
    def set_length(self, n: int) -> None:
        assert 0 <= n <= self.capacity, f"length {n} outside the capacity {self.capacity}"
        self.n_keys.fill_(int(n))

    def set_rope_delta(self, delta: int) -> None:
        """Set the position offset from the host.  The tensor is made on the first call: make it before a step is captured."""
        if self.rope_delta is None:
            self.rope_delta = torch.zeros((1,), dtype=torch.int32, device=self.n_keys.device)
        self.rope_delta.fill_(int(delta))

    # ---- the generation step: capturable ----
    def advance(self, R: int = 1) -> None:
        """n_keys += R on the device: once per step, before the layers."""
        self.n_keys.add_(int(R))

    def _q(self, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        return qkv[:, :heads * self.head_dim].view(qkv.shape[0], heads, self.head_dim)


class Fp8KVCache(_DeviceLengthCache):
    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, kv_scales: Sequence[torch.Tensor],
                 cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], device, dtype: torch.dtype,
                 rope_delta: Optional[int] = None):
        """kv_scales: per layer a float32 [2 * kv_heads] tensor (K scales then V scales; a [layers, 2 * kv_heads] tensor works).
        cos / sin: the RoPE tables [rows, head_dim] in ``dtype`` (contiguous), or both None for a model without rotation at this
        point.  rope_delta: the initial position offset; None = no offset tensor at all (``set_rope_delta`` makes one later)."""
        assert len(kv_scales) == layers
        self.scales = [s.to(device=torch.device(device), dtype=torch.float32).contiguous() for s in kv_scales]
        for s in self.scales:
            assert s.numel() == 2 * kv_heads
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, torch.float8_e4m3fn, rope_delta)

    def fill(self, layer: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write: kv_cols [T, 2 * kv_heads, head_dim] (K already rotated; the K|V columns of the fused q|k|v output work
        in place) into rows [0, T) of the layer's cache.  The length is set by ``set_length``, once for all layers."""
        T = kv_cols.shape[0]
        assert T <= self.capacity and tuple(kv_cols.shape[1:]) == (2 * self.kv_heads, self.head_dim)
        return ops.kv_quant_fp8(kv_cols, self.scales[layer], out=self.caches[layer][:T])

    def _append(self, layer: int, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        ops.kv_append_rope_fp8(qkv, heads, self.caches[layer], self.scales[layer], self.cos, self.sin, n_keys=self.n_keys,
                               rope_delta=self.rope_delta)
        return self._q(qkv, heads)

    def step(self, layer: int, qkv: torch.Tensor, heads: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """qkv [R, (heads + 2 * kv_heads) * head_dim], the raw projection of the R newest positions (``advance(R)`` came first):
        rotated and appended in place, then attended over the first n_keys rows -> [R, heads * head_dim]."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_fp8kv(q, self.caches[layer], self.scales[layer], n_keys=self.n_keys, causal=causal, out=out)

    def step_quant_i8(self, layer: int, qkv: torch.Tensor, heads: int, scale0: float, scale1: Optional[float] = None, *,
                      causal: bool = True, row_sel: Optional[torch.Tensor] = None, out=None, tiled: bool = False):
        """``step`` with the next Linear's static int8 quantizer fused into the attention's store (``ops.attn_decode_quant_i8``)."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_quant_i8(q, self.caches[layer], self.scales[layer], scale0, scale1, n_keys=self.n_keys, causal=causal,
                                        row_sel=row_sel, out=out, tiled=tiled)


class KVCache16(_DeviceLengthCache):
    def __init__(self, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, rope_delta: Optional[int] = None):
        """``Fp8KVCache`` without scales: the caches hold ``dtype`` (fp16 / bf16).  cos / sin, rope_delta: as there."""
        assert dtype in (torch.float16, torch.bfloat16)
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, dtype, rope_delta)

    def fill(self, layer: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write: a bit copy of kv_cols [T, 2 * kv_heads, head_dim] (``dtype``; K already rotated; a strided view of
        the fused q|k|v output works) into rows [0, T) of the layer's cache.  The length is set by ``set_length``."""
        T = kv_cols.shape[0]
        assert T <= self.capacity and tuple(kv_cols.shape[1:]) == (2 * self.kv_heads, self.head_dim) and kv_cols.dtype == self.dtype
        self.caches[layer][:T].copy_(kv_cols)
        return self.caches[layer][:T]

    def _append(self, layer: int, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        ops.kv_append_rope(qkv, heads, self.caches[layer], self.cos, self.sin, n_keys=self.n_keys, rope_delta=self.rope_delta)
        return self._q(qkv, heads)

    def step(self, layer: int, qkv: torch.Tensor, heads: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Fp8KVCache.step`` over the 16-bit cache: ``ops.kv_append_rope``, then ``ops.attn_decode``."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode(q, self.caches[layer], n_keys=self.n_keys, causal=causal, out=out)

    def step_quant_i8(self, layer: int, qkv: torch.Tensor, heads: int, scale0: float, scale1: Optional[float] = None, *,
                      causal: bool = True, row_sel: Optional[torch.Tensor] = None, out=None, tiled: bool = False):
        """``step`` with the next Linear's static int8 quantizer fused into the attention's store (``ops.attn_decode_quant_i8``)."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_quant_i8(q, self.caches[layer], None, scale0, scale1, n_keys=self.n_keys, causal=causal,
                                        row_sel=row_sel, out=out, tiled=tiled)


# ---- B sequences that step together: one buffer per layer, B lengths, B offsets ----
class _DeviceLengthCacheBatch(_DeviceLengthCache):
    """What the two batched cache classes share.  The single-sequence classes with a leading batch dimension: per layer ONE buffer
    ``[B, capacity, 2 * kv_heads, head_dim]``, ``n_keys`` int32 ``[B]`` and an optional ``rope_delta`` int32 ``[B]`` (every sequence
    has its own image, hence its own offset), all on the device.  All sequences advance together (``advance`` is the base's: one
    in-place add on the B lengths); ``step`` is one batched append and one batched attention over qkv ``[B * R, ...]`` (rows
    [b R, (b + 1) R) belong to sequence b), each reading the B lengths itself.  The same contract: after one warm-up ``advance`` and
    ``step`` with ``out`` neither synchronise nor allocate."""

    def __init__(self, batch: int, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, storage: torch.dtype, rope_delta: Optional[Sequence[int]]):
        assert batch >= 1
        self.batch = batch
        super().__init__(layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, storage, rope_delta, batch=batch)

    # ---- host side: bookkeeping (not for a captured step) ----
    def _per_sequence(self, values: Sequence[int], into: torch.Tensor) -> None:
        values = [int(v) for v in values]
        assert len(values) == self.batch, f"{len(values)} values for a batch of {self.batch} sequences"
        into.copy_(torch.tensor(values, dtype=torch.int32))

    def set_length(self, lengths: Sequence[int]) -> None:
        assert all(0 <= int(n) <= self.capacity for n in lengths), f"lengths {list(lengths)} outside the capacity {self.capacity}"
        self._per_sequence(lengths, self.n_keys)

    def set_rope_delta(self, deltas: Sequence[int]) -> None:
        """Set the B position offsets from the host.  The tensor is made on the first call: make it before a step is captured."""
        if self.rope_delta is None:
            self.rope_delta = torch.zeros((self.batch,), dtype=torch.int32, device=self.n_keys.device)
        self._per_sequence(deltas, self.rope_delta)

    def _q(self, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        return qkv[:, :heads * self.head_dim].view(self.batch, qkv.shape[0] // self.batch, heads, self.head_dim)


class Fp8KVCacheBatch(_DeviceLengthCacheBatch):
    def __init__(self, batch: int, layers: int, capacity: int, kv_heads: int, head_dim: int, kv_scales: Sequence[torch.Tensor],
                 cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], device, dtype: torch.dtype,
                 rope_delta: Optional[Sequence[int]] = None):
        """``Fp8KVCache`` for ``batch`` sequences.  kv_scales: per layer a float32 [2 * kv_heads] tensor, shared by the sequences (the
        scales are calibrated per layer, not per request).  rope_delta: the B initial offsets, or None."""
        assert len(kv_scales) == layers
        self.scales = [s.to(device=torch.device(device), dtype=torch.float32).contiguous() for s in kv_scales]
        for s in self.scales:
            assert s.numel() == 2 * kv_heads
        super().__init__(batch, layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, torch.float8_e4m3fn, rope_delta)

    def fill(self, layer: int, b: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write of sequence b: kv_cols [T, 2 * kv_heads, head_dim] (K already rotated) into rows [0, T) of its cache."""
        T = kv_cols.shape[0]
        assert T <= self.capacity and tuple(kv_cols.shape[1:]) == (2 * self.kv_heads, self.head_dim)
        return ops.kv_quant_fp8(kv_cols, self.scales[layer], out=self.caches[layer][b, :T])

    def _append(self, layer: int, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        ops.kv_append_rope_fp8_batch(qkv, heads, self.caches[layer], self.scales[layer], self.cos, self.sin, n_keys=self.n_keys,
                                     rope_delta=self.rope_delta)
        return self._q(qkv, heads)

    def step(self, layer: int, qkv: torch.Tensor, heads: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """qkv [B * R, (heads + 2 * kv_heads) * head_dim], the raw projection of every sequence's R newest positions (``advance(R)``
        came first): rotated and appended in place, then attended over each sequence's own n_keys rows -> [B * R, heads * head_dim]."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_fp8kv_batch(q, self.caches[layer], self.scales[layer], n_keys=self.n_keys, causal=causal, out=out)

    def step_quant_i8(self, layer: int, qkv: torch.Tensor, heads: int, scale0: float, scale1: Optional[float] = None, *,
                      causal: bool = True, row_sel: Optional[torch.Tensor] = None, out=None, tiled: bool = False):
        """``step`` with the next Linear's static int8 quantizer fused into the attention's store (``ops.attn_decode_quant_i8_batch``)."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_quant_i8_batch(q, self.caches[layer], self.scales[layer], scale0, scale1, n_keys=self.n_keys,
                                              causal=causal, row_sel=row_sel, out=out, tiled=tiled)


class KVCache16Batch(_DeviceLengthCacheBatch):
    def __init__(self, batch: int, layers: int, capacity: int, kv_heads: int, head_dim: int, cos: Optional[torch.Tensor],
                 sin: Optional[torch.Tensor], device, dtype: torch.dtype, rope_delta: Optional[Sequence[int]] = None):
        """``KVCache16`` for ``batch`` sequences: the caches hold ``dtype`` (fp16 / bf16), no scales."""
        assert dtype in (torch.float16, torch.bfloat16)
        super().__init__(batch, layers, capacity, kv_heads, head_dim, cos, sin, device, dtype, dtype, rope_delta)

    def fill(self, layer: int, b: int, kv_cols: torch.Tensor) -> torch.Tensor:
        """The prefill write of sequence b: a bit copy of kv_cols [T, 2 * kv_heads, head_dim] into rows [0, T) of its cache."""
        T = kv_cols.shape[0]
        assert T <= self.capacity and tuple(kv_cols.shape[1:]) == (2 * self.kv_heads, self.head_dim) and kv_cols.dtype == self.dtype
        self.caches[layer][b, :T].copy_(kv_cols)
        return self.caches[layer][b, :T]

    def _append(self, layer: int, qkv: torch.Tensor, heads: int) -> torch.Tensor:
        ops.kv_append_rope_batch(qkv, heads, self.caches[layer], self.cos, self.sin, n_keys=self.n_keys, rope_delta=self.rope_delta)
        return self._q(qkv, heads)

    def step(self, layer: int, qkv: torch.Tensor, heads: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Fp8KVCacheBatch.step`` over the 16-bit caches: ``ops.kv_append_rope_batch``, then ``ops.attn_decode_batch``."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_batch(q, self.caches[layer], n_keys=self.n_keys, causal=causal, out=out)

    def step_quant_i8(self, layer: int, qkv: torch.Tensor, heads: int, scale0: float, scale1: Optional[float] = None, *,
                      causal: bool = True, row_sel: Optional[torch.Tensor] = None, out=None, tiled: bool = False):
        """``step`` with the next Linear's static int8 quantizer fused into the attention's store (``ops.attn_decode_quant_i8_batch``)."""
        q = self._append(layer, qkv, heads)
        return ops.attn_decode_quant_i8_batch(q, self.caches[layer], None, scale0, scale1, n_keys=self.n_keys, causal=causal,
                                              row_sel=row_sel, out=out, tiled=tiled)
