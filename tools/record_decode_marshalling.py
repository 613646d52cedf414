#!/usr/bin/env python3
"""Write tests/golden/decode_marshalling.json: what the twelve public ops of a generation step hand to the C ABI for the calls of
tests/decode_marshalling_cases.py (entry point and arguments; addresses by the name of the tensor they belong to).  Nothing is
launched.  Record it at the commit whose marshalling is to be kept, then change the wrappers: tests/test_gpu_decode_marshalling.py
holds them to the file.
usage (GPU box): python3 tools/record_decode_marshalling.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from decode_marshalling_cases import record  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "decode_marshalling.json")


def main():
    calls = record()
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in calls) + "\n]\n")
    print(f"{len(calls)} calls of {len({c['entry'] for c in calls})} entry points -> {OUT}")


if __name__ == "__main__":
    main()
