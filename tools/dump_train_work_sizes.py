#!/usr/bin/env python3
"""Record what the seven size queries of the training work buffers answer over the grid of tests/train_work_grid.py into
tests/golden/train_work_sizes.json (one row per net and shape: the NetConfig constructor arguments, batch, frames and the
sizes in the order of train_work_grid.QUERIES).  Host arithmetic only: no GPU is needed.

The fixture pins these sizes to the commit it was recorded at (tests/test_train_work_host.py), so run this against a
library built from THAT commit - SWN_HIP_LIB=/path/to/libswn_hip.so selects it - and only when a size is meant to change.

    SWN_HIP_LIB=/path/to/parent/libswn_hip.so python tools/dump_train_work_sizes.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_work_sizes.json"))
    args = ap.parse_args()
    import ctypes

    import train_work_grid as G
    from shallow_wavenet_amd import _lib
    # the library alone (no torch, no device): the queries are host arithmetic
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for q in G.QUERIES:
        getattr(lib, q).restype, getattr(lib, q).argtypes = _lib.SIGNATURES[q]
    rows = G.rows(lib)
    with open(args.out, "w") as f:
        f.write('{"queries": ' + json.dumps(list(G.QUERIES)) + ',\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{len(rows)} rows from {_lib.LIB_PATH} -> {args.out}")


if __name__ == "__main__":
    main()
