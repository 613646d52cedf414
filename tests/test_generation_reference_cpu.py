"""Pins tests/generation_reference.py -- the float64 model of generation -- and the inputs of
tests/test_gpu_generation_reference.py, on the CPU alone.  Three conditions make the GPU file's demands fair, and each is
asserted here for every case, storage and sequence of ``CASES``:

  the mutation gap   C * E_plain <= E_mut / 5: honest 16-bit arithmetic (``plain``) sits C times closer to the reference than the
                     nearest mistake of ``MUTATIONS`` does after a further factor 5 (C is per dtype).  A mutation a sequence cannot
                     see is named by ``_unseen`` below with its reason, and asserted to move nothing: never skipped silently.  A
                     sequence without the gap is named in its case's ``no_gap`` and asserted to lack it;
  16-bit margins     every float64 top-1 / top-2 margin is >= 4 * plain's largest logit error, so the whole id sequence of float64
                     greedy decoding is a fair demand;
  e4m3 quarter cap   with plain's greedy decoding as the stand-in for the device and the reference forced on plain's cache, at most
                     a quarter of the generated positions have a margin below 4 * plain's logit error, and every other position
                     matches the float64 argmax.

And the checker itself has no off-by-one: evaluated position by position it equals the whole-sequence evaluation to 1e-12."""
import pytest
import torch

import generation_reference as G

torch.set_grad_enabled(False)


def _seqs(case):
    return range(len(G.CASES[case].sequences))


def _unseen(case, storage, seq):
    """the mutations that cannot move this sequence's hidden states, each with its reason"""
    c = G.CASES[case]
    out = {}
    if c.sequences[seq].rope_delta == 0:
        out["rope_delta_ignored"] = "this sequence's rope_delta is 0"
    if c.geometry.heads == c.geometry.kv_heads:
        out["gqa_modulo"] = "one KV head per query head: h % kv_heads == h // 1"
    if storage == "16bit":
        out["kv_scale_halves_swapped"] = "a 16-bit cache has no scales"
    else:
        out["kv_scale_halves_swapped"] = "the attention reads the forced cache; the reference's own codes show it (asserted below)"
    return out


@pytest.mark.parametrize("storage", G.STORAGES)
def test_incremental_evaluation_equals_the_whole_sequence(storage):
    for name in ("h4kv2d128-fp16", "h4kv4d64-fp16"):
        c, w = G.CASES[name], G.case_weights(name)
        kw = {"storage": storage, "kv_scales": G.make_kv_scales(c.geometry) if storage == "e4m3" else None}
        for P, delta in [(5, 3), (2, -2)]:
            ids = G.make_prompt(11, P + 7)
            whole = G.reference(w, ids, P, delta, **kw)
            hidden, logits = G.reference_incremental(w, ids, P, delta, **kw)
            assert G.rel_rows(hidden, whole["hidden"]).max() <= 1e-12, (name, P, delta)
            assert G.rel_rows(logits, whole["logits"]).max() <= 1e-12, (name, P, delta)


@pytest.mark.parametrize("storage", G.STORAGES)
@pytest.mark.parametrize("case", list(G.CASES))
def test_mutation_gap(case, storage):
    for seq in _seqs(case):
        y, errs, unseen = G.yardstick(case, storage, seq), G.mutation_errors(case, storage, seq), _unseen(case, storage, seq)
        for m in unseen:
            assert errs[m] <= 1e-12, f"{case} {storage} seq {seq}: {m} is listed as unseen but moves the hidden state by {errs[m]:.2e}"
        seen = {m: e for m, e in errs.items() if m not in unseen}
        assert len(seen) >= 4
        e_mut = min(seen.values())
        print(f"{case} {storage} seq {seq}: E_plain {y['e_plain']:.2e} E_mut {e_mut:.2e} ({min(seen, key=seen.get)}) "
              f"limit of c {e_mut / 5 / y['e_plain']:.1f} unseen {sorted(unseen)}")
        holds = G.C[G.CASES[case].dtype] * y["e_plain"] <= e_mut / 5
        if (storage, seq) in G.CASES[case].no_gap:                    # a named exemption, and a needed one
            assert not holds, f"{case} {storage} seq {seq} is listed in no_gap but has the gap: take it off the list"
        else:
            assert holds, (case, storage, seq, y["e_plain"], seen)


@pytest.mark.parametrize("case", list(G.CASES))
def test_swapped_scale_halves_show_in_the_codes(case):
    """the one mutation the forced e4m3 reference cannot see in a hidden state: its own codes then differ from plain's cache far
    beyond the 2 x plain's share the GPU file allows"""
    c, w = G.CASES[case], G.case_weights(case)
    HKV = c.geometry.kv_heads
    for seq in _seqs(case):
        y, s = G.yardstick(case, "e4m3", seq), c.sequences[seq]
        mut = G.reference(w, y["ids"][:-1], s.prompt_len, s.rope_delta, forced_cache=y["forced"], mutation="kv_scale_halves_swapped", **y["kw"])
        for i in range(G.LAYERS):
            for half, sl in enumerate((slice(0, HKV), slice(HKV, 2 * HKV))):
                share = G.share_differing(y["plain"]["codes"][i][:, sl], mut["codes"][i][:, sl])
                assert share > 0.5 > 4 * y["share"][i][half], (case, seq, i, half, share, y["share"][i])


@pytest.mark.parametrize("case", list(G.CASES))
def test_16bit_margins_make_the_id_sequence_a_fair_demand(case):
    for seq in _seqs(case):
        y = G.yardstick(case, "16bit", seq)
        assert len(y["margin"]) == G.STEPS + 1
        print(f"{case} seq {seq}: min margin {float(y['margin'].min()):.4f} plain logit error {y['logit_err']:.4f}")
        assert float(y["margin"].min()) >= 4 * y["logit_err"], (case, seq)
        P = G.CASES[case].sequences[seq].prompt_len
        assert torch.argmax(y["plain"]["logits"][P - 1:], dim=1).tolist() == y["ids"][P:], (case, seq)      # so plain decodes them too


@pytest.mark.parametrize("case", list(G.CASES))
def test_e4m3_quarter_cap_with_plain_as_the_device(case):
    for seq in _seqs(case):
        y = G.yardstick(case, "e4m3", seq)
        P = G.CASES[case].sequences[seq].prompt_len
        low = y["margin"] < 4 * y["logit_err"]
        print(f"{case} seq {seq}: {int(low.sum())} of {len(low)} margins under 4 x {y['logit_err']:.4f}; code shares {y['share']}")
        assert int(low.sum()) <= G.STEPS // 4, (case, seq)
        want = G.margins(y["ref"]["logits"][P - 1:])[0]
        for j, (a, b) in enumerate(zip(want, y["ids"][P:])):
            assert low[j] or a == b, (case, seq, j)
