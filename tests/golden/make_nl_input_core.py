"""Records tests/golden/nl_input_core.npz: the bits of pasnl_cls_nl_cell_input and pasnl_cls_nl_cell_input_grad for the shapes of
tests/nl_input_core_cases.py, as the library of the checked-out commit computes them on an MI355X, and that commit's hash.

It was run on the commit before the two kernels' shared machinery moved into csrc/nl_input_core.hpp (no arithmetic did);
tests/test_gpu_nl_input_parent_bits.py holds every later build to those bits.  Run it again only on a commit whose arithmetic is
meant to become the new reference:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_nl_input_core.py $(git rev-parse HEAD) [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import nl_cell_input_grad_ref as R  # noqa: E402
import nl_input_core_cases as C  # noqa: E402
from guarded import NAN_BYTE, WS_BYTE  # noqa: E402


def main(commit, path):
    from pointasnl_amd import _hip

    _hip.lib()
    _hip.require_device()
    rec = {"commit": np.array(commit)}
    for shape in C.SHAPES:
        h, g = R.problem(*shape)
        out = C.run_forward(shape, h, NAN_BYTE)
        full = C.run_grad(shape, h, g, R.NAMES, NAN_BYTE, WS_BYTE)
        subsets = {name: C.run_grad(shape, h, g, need, NAN_BYTE, WS_BYTE) for name, need in C.SUBSETS.items()} if shape in C.ABI_SHAPES else {}
        for name, a in C.record(out, full, subsets).items():
            rec[f"{C.shape_id(shape)}/{name}"] = a
    np.savez(path, **rec)
    print(f"{path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "nl_input_core.npz"))
