"""What the twelve public ops of a generation step hand to the C ABI, held to tests/golden/decode_marshalling.json (written by
tools/record_decode_marshalling.py before the Python layer of the step was consolidated): the entry point and every argument of
every call of tests/decode_marshalling_cases.py -- the stride passed for a dimension of size 1, which calls get a workspace, which
integers become device tensors.  The result tests cannot see these; nothing is launched here."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_marshalling.json")


def test_every_call_reaches_the_entry_point_with_the_recorded_arguments():
    from decode_marshalling_cases import record
    from mquant_amd import _lib
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record()))
    assert [c["call"] for c in got] == [c["call"] for c in want]
    for g, w in zip(got, want):
        assert g == w, g["call"]
    entries = {c["entry"] for c in want}               # twelve ops; the two fused ones choose between two entry points each
    assert len(entries) == 14 and all(len(c["args"]) == len(_lib.SIGNATURES[c["entry"]][1]) for c in want)
