"""A greedy generation loop that never leaves the device: the step feeds itself.

``Fp8KVCache`` and ``KVCache16`` made the middle of a generation step capturable (the length lives on the device); ``GreedyLoop`` closes both ends with
ONE int32 ``token`` on the device, as ``n_keys`` already is:

    cache.advance(1)                                             # n_keys += 1
    hidden = embed_tokens[token]; ids[n_keys - 1] = token        # ops.embed_gather: the id and the position are read on the device
    h = body(hidden)                                             # the decoder layers; they call cache.step / cache.step_quant_i8
    h = rms_norm(h)                                              # weight-less: a norm weight is folded into lm_head
    token = argmax(h @ lm_head.t())                              # ops.gemv_f16_argmax: no logits leave the chip

One linear chain of launches, captured once and replayed N times for N tokens; the host reads the ids afterwards from the log,
which is indexed by cache position -- one copy, the single synchronisation.  Greedy selection only: no sampling, no EOS handling
(inspect the ids between batches of replays)."""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch
import torch.nn.functional as F

from . import ops
from .kv_cache import Fp8KVCache, KVCache16


class GreedyLoop:
    def __init__(self, cache: Union[Fp8KVCache, KVCache16], embed_tokens: torch.Tensor, lm_head: torch.Tensor,
                 body: Callable[[torch.Tensor], torch.Tensor], eps: float = 1e-6):
        """cache: either cache class -- the loop touches ``dtype``, ``capacity``, ``n_keys``, ``caches``, ``advance`` and ``set_length``
        only, and the body calls the cache's own ``step``.  embed_tokens [vocab, dim] and lm_head [vocab_out, dim]: fp16 / bf16 CUDA tensors of the cache's dtype.  body: hidden
        [1, dim] -> [1, dim], the decoder layers of ONE new position; for a step that is to be captured it must neither synchronise
        nor depend on host state that changes between steps."""
        assert embed_tokens.dim() == 2 and lm_head.dim() == 2 and embed_tokens.shape[1] == lm_head.shape[1]
        assert embed_tokens.dtype == lm_head.dtype == cache.dtype and embed_tokens.device == lm_head.device == cache.n_keys.device
        self.cache, self.embed_tokens, self.lm_head, self.body, self.eps = cache, embed_tokens, lm_head, body, eps
        self.dim = embed_tokens.shape[1]
        dev = embed_tokens.device
        self.token = torch.zeros((1,), dtype=torch.int32, device=dev)              # the id the next step embeds
        self.ids = torch.zeros((cache.capacity,), dtype=torch.int32, device=dev)   # ids[t] = the id embedded at cache position t
        self.hidden = torch.empty((1, self.dim), dtype=embed_tokens.dtype, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.pos = 0                 # host side: the cache position of the next step (the host issues the steps, so it knows)

    def start(self, prompt_len: int, first_token: int) -> None:
        """The prefill wrote cache rows [0, prompt_len) and picked first_token: the next step embeds it at position prompt_len."""
        assert 0 <= prompt_len < self.cache.capacity, f"prompt_len {prompt_len} leaves no room in a cache of {self.cache.capacity} rows"
        self.cache.set_length(prompt_len)
        self.token.fill_(int(first_token))
        self.pos = prompt_len

    def step(self) -> None:
        """One position, on the current stream: capturable (after one warm-up step it neither allocates outside torch's own ops nor
        synchronises).  Does not move ``pos``: ``generate`` counts the steps."""
        self.cache.advance(1)
        ops.embed_gather(self.embed_tokens, self.token, out=self.hidden, id_log=self.ids, n_keys=self.cache.n_keys)
        h = self.body(self.hidden)
        h = F.rms_norm(h, (self.dim,), eps=self.eps)
        ops.gemv_f16_argmax(h, self.lm_head, token_out=self.token)

    def capture(self) -> None:
        """Warm up (workspaces, one-time checks) and capture ``step`` once, on a side stream.  Everything the warm-up step wrote is
        restored afterwards -- ``n_keys``, ``token``, the cache row and the log entry of its position -- so this may come before
        or after ``start`` and before or after the prefill.  Set-up, not the loop: it reads ``n_keys`` back once."""
        n_keys, token = self.cache.n_keys.clone(), self.token.clone()
        at = min(max(int(n_keys.item()) + 1, 1), self.cache.capacity) - 1          # the position the kernels' clamp gives the warm-up
        rows, logged = [c[at].clone() for c in self.cache.caches], self.ids[at].clone()
        side = torch.cuda.Stream(device=self.token.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.step()
        torch.cuda.current_stream().wait_stream(side)
        self.cache.n_keys.copy_(n_keys)
        self.token.copy_(token)
        self.ids[at].copy_(logged)
        for c, row in zip(self.cache.caches, rows):
            c[at].copy_(row)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self.step()
        self.graph = graph

    def generate(self, n: int) -> torch.Tensor:
        """n more positions (graph replays once captured, eager steps before) -> the ids embedded at them, an int32 CPU tensor [n]:
        after ``start`` entry 0 is first_token, and the n-th generated id is left in ``token``.  The copy is the only synchronisation."""
        assert n >= 0 and self.pos + n <= self.cache.capacity, f"{n} steps from position {self.pos} exceed the cache's {self.cache.capacity} rows"
        run = self.graph.replay if self.graph is not None else self.step
        for _ in range(n):
            run()
        first, self.pos = self.pos, self.pos + n
        return self.ids[first:first + n].cpu()
