"""A greedy generation loop that never leaves the device: the step feeds itself.

The cache classes made the middle of a generation step capturable (the length lives on the device); the loop closes both ends with
ONE int32 ``token`` on the device, as ``n_keys`` already is:

    cache.advance(1)                                             # n_keys += 1
    hidden = embed_tokens[token]; ids[n_keys - 1] = token        # ops.embed_gather: the id and the position are read on the device
    h = body(hidden)                                             # the decoder layers; they call cache.step / cache.step_quant_i8
    h = rms_norm(h)                                              # weight-less: a norm weight is folded into lm_head
    token = argmax(h @ lm_head.t())                              # ops.gemv_f16_argmax: no logits leave the chip

One linear chain of launches, captured once and replayed N times for N tokens; the host reads the ids afterwards from the log,
which is indexed by cache position -- one copy, the single synchronisation.  Greedy selection only: no sampling, no EOS handling
(inspect the ids between batches of replays).

``_GreedyLoop`` holds the step, its capture and the replay loop once, over B sequences: ``GreedyLoopBatch`` is it for the batched
caches, and ``GreedyLoop`` is it for one sequence, which the shared code sees as a batch of one through views (``ids[None]``,
``cache[None]``) while ``token`` [1], ``ids`` [capacity], ``pos`` (an int) and the gather op (``ops.embed_gather``) stay the single
sequence's own."""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch
import torch.nn.functional as F

from . import ops
from .kv_cache import Fp8KVCache, Fp8KVCacheBatch, KVCache16, KVCache16Batch


class _GreedyLoop:
    def __init__(self, cache, embed_tokens: torch.Tensor, lm_head: torch.Tensor, body: Callable[[torch.Tensor], torch.Tensor], eps: float,
                 batch: Optional[int]):
        """batch: None = one sequence (``token`` [1], ``ids`` [capacity], ``pos`` an int), B = a batched cache's B sequences
        (``token`` [B], ``ids`` [B, capacity], ``pos`` a list)."""
        assert embed_tokens.dim() == 2 and lm_head.dim() == 2 and embed_tokens.shape[1] == lm_head.shape[1]
        assert embed_tokens.dtype == lm_head.dtype == cache.dtype and embed_tokens.device == lm_head.device == cache.n_keys.device
        self.cache, self.embed_tokens, self.lm_head, self.body, self.eps = cache, embed_tokens, lm_head, body, eps
        self.dim = embed_tokens.shape[1]
        dev, lead = embed_tokens.device, () if batch is None else (batch,)
        self.token = torch.zeros(lead or (1,), dtype=torch.int32, device=dev)             # the id(s) the next step embeds
        self.ids = torch.zeros(lead + (cache.capacity,), dtype=torch.int32, device=dev)   # ids[(b,) t] = the id embedded at cache position t
        self.hidden = torch.empty((batch or 1, self.dim), dtype=embed_tokens.dtype, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.pos = 0 if batch is None else [0] * batch   # host side: the cache position of the next step (the host issues the steps, so it knows)
        self._batched, self._gather = batch is not None, ops.embed_gather if batch is None else ops.embed_gather_batch

    def _by_sequence(self, t: torch.Tensor) -> torch.Tensor:
        """The log or a cache as [sequence, position, ...]: one sequence is a batch of one."""
        return t if self._batched else t[None]

    def step(self) -> None:
        """One position (of every sequence), on the current stream: capturable (after one warm-up step it neither allocates outside
        torch's own ops nor synchronises).  Does not move ``pos``: ``generate`` counts the steps."""
        self.cache.advance(1)
        self._gather(self.embed_tokens, self.token, out=self.hidden, id_log=self.ids, n_keys=self.cache.n_keys)
        h = self.body(self.hidden)
        h = F.rms_norm(h, (self.dim,), eps=self.eps)
        ops.gemv_f16_argmax(h, self.lm_head, token_out=self.token)

    def capture(self) -> None:
        """Warm up (workspaces, one-time checks) and capture ``step`` once, on a side stream.  Everything the warm-up step wrote is
        restored afterwards -- ``n_keys``, ``token`` and, for every sequence, the cache row and the log entry of its own position --
        so this may come before or after ``start`` and before or after the prefill.  Set-up, not the loop: it reads ``n_keys`` back
        once."""
        n_keys, token = self.cache.n_keys.clone(), self.token.clone()
        at = [min(max(n + 1, 1), self.cache.capacity) - 1 for n in n_keys.cpu().tolist()]     # the positions the kernels' clamps give the warm-up
        seqs = list(range(len(at)))
        caches, ids = [self._by_sequence(c).view(torch.uint8) for c in self.cache.caches], self._by_sequence(self.ids)
        rows, logged = [c[seqs, at] for c in caches], ids[seqs, at]                           # copies (indexed by lists)
        side = torch.cuda.Stream(device=self.token.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.step()
        torch.cuda.current_stream().wait_stream(side)
        self.cache.n_keys.copy_(n_keys)
        self.token.copy_(token)
        ids[seqs, at] = logged
        for c, row in zip(caches, rows):
            c[seqs, at] = row
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self.step()
        self.graph = graph

    def generate(self, n: int) -> torch.Tensor:
        """n more positions (graph replays once captured, eager steps before) -> the ids embedded at them, an int32 CPU tensor [n]
        (B sequences: [B, n], row b from sequence b's own position on): after ``start`` entry 0 is the first token, and the n-th
        generated id is left in ``token``.  The copy is the only synchronisation."""
        first = self.pos if self._batched else [self.pos]
        assert n >= 0 and max(first) + n <= self.cache.capacity, f"{n} steps from position {self.pos} exceed the cache's {self.cache.capacity} rows"
        run = self.graph.replay if self.graph is not None else self.step
        for _ in range(n):
            run()
        if not self._batched:
            self.pos += n
            return self.ids[first[0]:first[0] + n].cpu()
        self.pos = [p + n for p in first]
        ids = self.ids.cpu()
        return torch.stack([ids[b, p:p + n] for b, p in enumerate(first)])


class GreedyLoop(_GreedyLoop):
    def __init__(self, cache: Union[Fp8KVCache, KVCache16], embed_tokens: torch.Tensor, lm_head: torch.Tensor,
                 body: Callable[[torch.Tensor], torch.Tensor], eps: float = 1e-6):
        """cache: either single-sequence cache class -- the loop touches ``dtype``, ``capacity``, ``n_keys``, ``caches``, ``advance`` and
        ``set_length`` only, and the body calls the cache's own ``step``.  embed_tokens [vocab, dim] and lm_head [vocab_out, dim]:
        fp16 / bf16 CUDA tensors of the cache's dtype.  body: hidden [1, dim] -> [1, dim], the decoder layers of ONE new position; for
        a step that is to be captured it must neither synchronise nor depend on host state that changes between steps."""
        super().__init__(cache, embed_tokens, lm_head, body, eps, None)

    def start(self, prompt_len: int, first_token: int) -> None:
        """The prefill wrote cache rows [0, prompt_len) and picked first_token: the next step embeds it at position prompt_len."""
        assert 0 <= prompt_len < self.cache.capacity, f"prompt_len {prompt_len} leaves no room in a cache of {self.cache.capacity} rows"
        self.cache.set_length(prompt_len)
        self.token.fill_(int(first_token))
        self.pos = prompt_len


class GreedyLoopBatch(_GreedyLoop):
    """``GreedyLoop`` for B <= 8 sequences that step together over a batched cache: one weight pass of the body (hidden [B, dim] ->
    [B, dim]; it calls the batched cache's step) and of lm_head (``ops.gemv_f16_argmax`` at M = B) serves B tokens; the gather is
    ``ops.embed_gather_batch``.  All sequences step together: no stop ids, no per-sequence masks, no sampling."""

    def __init__(self, cache: Union[Fp8KVCacheBatch, KVCache16Batch], embed_tokens: torch.Tensor, lm_head: torch.Tensor,
                 body: Callable[[torch.Tensor], torch.Tensor], eps: float = 1e-6):
        assert 1 <= cache.batch <= 8, f"a batch of {cache.batch} sequences (1 .. 8: the rows of ops.embed_gather_batch and ops.gemv_f16_argmax)"
        super().__init__(cache, embed_tokens, lm_head, body, eps, cache.batch)
        self.batch = cache.batch

    def start(self, prompt_lens, first_tokens) -> None:
        """The prefill wrote rows [0, prompt_lens[b]) of sequence b's caches and picked first_tokens[b]."""
        prompt_lens, first_tokens = [int(n) for n in prompt_lens], [int(t) for t in first_tokens]
        assert len(prompt_lens) == len(first_tokens) == self.batch, f"{self.batch} sequences need {self.batch} prompt lengths and first tokens"
        assert all(0 <= n < self.cache.capacity for n in prompt_lens), \
            f"prompt_lens {prompt_lens} leave no room in caches of {self.cache.capacity} rows"
        self.cache.set_length(prompt_lens)
        self.token.copy_(torch.tensor(first_tokens, dtype=torch.int32))
        self.pos = prompt_lens
