#!/usr/bin/env python3
"""Writes tests/golden/abi_refusals.json: return code and lft_last_error() text of every call in tests/abi_refusals_util.py, as the
built library (or the one LFT_LIB_PATH names) answers them.  None of the calls reaches the device, so this runs without a GPU.
Run it at the commit whose answers are to be kept -- before a change that moves argument checks, not after it;
tests/test_abi_refusals_host.py replays the table and requires the same answers."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from lft_amd import _lib            # noqa: E402
import abi_refusals_util as U       # noqa: E402

if __name__ == "__main__":
    if not os.environ.get("LFT_LIB_PATH"):
        _lib.build()
    records = U.replay(_lib.lib())
    path = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
    print(f"{path}: {len(records)} cases over {len({r['entry'] for r in records})} entry points, {sum(r['rc'] != 0 for r in records)} refused")
