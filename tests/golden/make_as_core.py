"""Records tests/golden/as_core.npz: the bits of the AdaptiveSampling cell's forward entries (pasnl_as_*) and of its fused
backward (pasnl_cls_as_*_grad) for the cases of tests/as_core_cases.py, as the library of the checked-out commit computes them on an
MI355X, and that commit's hash.

It was run on the commit before the forward moved into csrc/as_cell.hip and both directions onto csrc/as_core.hpp (no arithmetic
did); tests/test_gpu_as_core_parent_bits.py holds every later build to those bits.  A case enters the file only if, on the
recording build too, its guard bands were intact, a second run over other stale bytes gave the same bytes and every subset call
gave the full call's bits; the recorder stops otherwise.  Run it again only on a commit whose arithmetic is meant to become the
new reference:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_as_core.py $(git rev-parse HEAD) [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import as_core_cases as C  # noqa: E402
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE  # noqa: E402


def main(commit, path):
    from pointasnl_amd import _hip

    _hip.lib()
    _hip.require_device()
    rec = {"commit": np.array(commit)}
    for case in C.CASES:
        outs = C.run(case, NAN_BYTE, WS_BYTE)  # (asserts the guards)
        again = C.run(case, ALT_BYTE, ALT_WS_BYTE)
        for k, a in outs.items():
            assert np.isfinite(a).all() and again[k].tobytes() == a.tobytes(), (case, k)
        for need in C.SUBSETS.get(case[0], {}).values():
            part = C.run(case, NAN_BYTE, WS_BYTE, need)
            assert set(part) == set(need) and all(part[k].tobytes() == outs[k].tobytes() for k in need), (case, need)
        for name, a in C.record(outs).items():
            rec[f"{C.case_id(case)}/{name}"] = a
        print(C.case_id(case), "ok", flush=True)
    np.savez(path, **rec)
    print(f"{path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "as_core.npz"))
