"""Every forward entry point of include/pasnl.h (the model path and the input stage) held to its buffers: each case of
tests/abi_cases.py goes through the C ABI with every output a guarded view of exactly the bytes the header states and the
workspace a guarded view of exactly the bytes its size function returns (tests/guarded.py), twice -- over 0xFF outputs and a
0xA5 workspace, then over 0x5A outputs and a zeroed workspace.

After each run: PASNL_OK; every guard holds its fill; columns of a wider table that the entry does not own, rows past a count
and outputs the header calls ignored hold the fill of the run; the defined part equals the oracle the entry's parity test
uses, at that test's exactness or tolerance.  Between the runs the defined part is bit-identical: an element that was never
written differs, and so does a result that depends on what the workspace or the output held before the call.  With one byte
less workspace the entry answers PASNL_EWORKSPACE and touches nothing.

Every byte a kernel could reach by storing a row or a tile too far is memory the test owns."""
import ctypes

import numpy as np
import pytest
import torch

import abi_cases as A
from guarded import ALT_BYTE, ALT_WS_BYTE, GUARD, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

IDS = [c.id for c in A.CASES]
WITH_WS = [c for c in A.CASES if "workspace_bytes" in " ".join(c.uses) and not c.no_ws]

RUNS = (("A", NAN_BYTE, WS_BYTE), ("B", ALT_BYTE, ALT_WS_BYTE))


def scalar(a):
    if isinstance(a, A.L):
        return ctypes.c_long(int(a.v))
    if isinstance(a, A.F):
        return ctypes.c_float(float(a.v))
    if isinstance(a, A.D):
        return ctypes.c_double(float(a.v))
    if isinstance(a, (int, np.integer)):
        return int(a)
    return None


def size_of(fn, args):
    from pointasnl_amd import _hip

    return int(getattr(_hip.lib(), fn)(*[scalar(a) for a in args]))


def call(entry, args):
    from pointasnl_amd import _hip

    return getattr(_hip.lib(), entry)(*args, _hip.stream_ptr())


class Inputs:
    """the device copies of a case's inputs, made once and never written: ordinary tensors.  A Prep input is produced here, by
    its own entry point, into a guarded buffer of exactly the bytes the header states."""

    def __init__(self, built):
        self.keep, self.args = [], []
        for a in built.args:
            if isinstance(a, np.ndarray):
                self.args.append(self.tensor(a))
            elif isinstance(a, A.Prep):
                self.args.append(self.prepare(a))
            else:
                self.args.append(a)

    def tensor(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def prepare(self, prep):
        if prep.bytes_fn:
            assert size_of(prep.bytes_fn, prep.bytes_args) == prep.nbytes, prep.bytes_fn
        dst = Guarded(prep.nbytes, NAN_BYTE, output_guard(0))
        args = []
        for a in prep.args:
            if a is A.DST:
                args.append(ctypes.c_void_p(dst.ptr))
            elif isinstance(a, np.ndarray):
                args.append(self.tensor(a))
            else:
                args.append(scalar(a))
        assert call(prep.entry, args) == A.OK, prep.entry
        torch.cuda.synchronize()
        assert dst.guards_intact(), prep.entry
        self.keep.append(dst)
        return ctypes.c_void_p(dst.ptr)


def launch(entry, built, inputs, out_fill, ws_fill, short=0):
    """one call -> (status, {output: Guarded}, workspace Guarded or None)"""
    outs = {o.name: Guarded(o.nbytes, out_fill, output_guard(o.row_bytes)) for o in built.outs}
    ws, nbytes = None, 0
    if built.ws:
        nbytes = size_of(*built.ws)
        ws = Guarded(nbytes, ws_fill)
        if built.ws_zero:  # the part the header requires the caller to have zeroed
            assert built.ws_zero <= nbytes
            ws.inside()[:built.ws_zero] = 0
    args = []
    for a in inputs.args:
        if isinstance(a, A.Ref):
            o = next(o for o in built.outs if o.name == a.name)
            args.append(ctypes.c_void_p(outs[a.name].ptr + a.offset * np.dtype(o.dtype).itemsize))
        elif a is A.WS:
            args.append(ctypes.c_void_p(ws.ptr))
        elif a is A.WSB:
            args.append(ctypes.c_size_t(nbytes - short))
        elif a is None:
            args.append(ctypes.c_void_p(0))
        elif isinstance(a, ctypes.c_void_p):
            args.append(a)
        else:
            args.append(scalar(a))
    status = call(entry, args)
    torch.cuda.synchronize()
    return status, outs, ws


def bf16_planes(words):
    """(3, k / 8, n, 8) bf16 words in operand order -> (3, k, n) float64"""
    planes = (words.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return planes.transpose(0, 1, 3, 2).reshape(3, -1, words.shape[2])


def compare(o, got, want, defined):
    kind = o.cmp[0]
    if kind == "bf16x3":
        back = bf16_planes(got).sum(axis=0)
        w = want.astype(np.float64)
        worst = float((np.abs(back - w) / np.maximum(np.abs(w), 1e-30)).max())
        print(f"  {o.name}: largest |hi + mid + lo - w| / |w| = {worst:.3g}")
        assert worst <= 2.0 ** -23
        return
    g, w = got[defined], want[defined]
    if kind == "bits":
        np.testing.assert_array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8), err_msg=o.name)
        return
    assert np.isfinite(g).all(), o.name
    err = float(np.abs(g.astype(np.float64) - w).max())
    scale = float(np.abs(w).max())
    print(f"  {o.name}: largest error {err:.3g} at output scale {scale:.3g} ({o.cmp})")
    if kind == "allclose":
        np.testing.assert_allclose(g, w, rtol=o.cmp[1], atol=o.cmp[2], err_msg=o.name)
    elif kind == "scale":
        assert err <= o.cmp[1] * scale, o.name
    else:
        assert kind == "scale1" and err <= o.cmp[1] * max(1.0, scale), o.name


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_entry_stays_inside_its_buffers(case):
    built = case.built()
    inputs = Inputs(built)
    for o in built.outs:
        if o.bytes_fn:
            assert size_of(o.bytes_fn, o.bytes_args) == o.nbytes, o.bytes_fn
    if built.ws:
        assert (size_of(*built.ws) == 0) == case.no_ws, built.ws
    seen = {}
    for run, out_fill, ws_fill in RUNS:
        status, outs, ws = launch(case.entry, built, inputs, out_fill, ws_fill)
        assert status == A.OK, (run, status)
        if ws is not None:
            assert ws.guards_intact(), f"run {run}: bytes beside the workspace were written"
        for o in built.outs:
            buf = outs[o.name]
            assert buf.guards_intact(), f"run {run}: bytes beside {o.name} were written"
            got = buf.array(o.shape, o.dtype)
            st = o.states()
            kept = got[st == A.KEPT]
            assert (kept.view(np.uint8) == out_fill).all(), f"run {run}: {o.name} was written where the header says it is not"
            defined = st == A.DEFINED
            if defined.any():
                print(f"run {run}")
                compare(o, got, built.want[o.name], defined)
            seen[run, o.name] = got[defined].copy()
        got = {o.name: outs[o.name].array(o.shape, o.dtype) for o in built.outs}
        for name, ix, want in built.exact:
            np.testing.assert_array_equal(np.ascontiguousarray(got[name][ix]).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
        for a, ix, b in built.alias:
            np.testing.assert_array_equal(np.ascontiguousarray(got[a][ix]).view(np.uint8), got[b].view(np.uint8))
    for o in built.outs:
        np.testing.assert_array_equal(seen["A", o.name].view(np.uint8), seen["B", o.name].view(np.uint8),
                                      err_msg=f"{o.name} depends on what the buffers held before the call")


@pytest.mark.parametrize("case", WITH_WS, ids=[c.id for c in WITH_WS])
def test_one_byte_less_workspace_is_refused_and_nothing_is_touched(case):
    built = case.built()
    inputs = Inputs(built)
    assert size_of(*built.ws) > 0
    status, outs, ws = launch(case.entry, built, inputs, NAN_BYTE, WS_BYTE, short=1)
    assert status == A.EWORKSPACE
    if built.ws_zero:
        assert ws.guards_intact() and bool((ws.inside()[built.ws_zero:] == WS_BYTE).all()) and not bool(ws.inside()[:built.ws_zero].any())
    else:
        assert ws.untouched()
    for o in built.outs:
        assert outs[o.name].untouched(), o.name


def test_guards_are_sized_as_stated():
    """an output's guard is the larger of 4 KiB and one output row, rounded up to 256 bytes; the view keeps its alignment"""
    assert GUARD == 256 and output_guard(12) == 4096 and output_guard(4097) == 4352 and output_guard(16384 * 4) == 65536
    g = Guarded(100, NAN_BYTE, output_guard(5000))
    assert g.guard == 5120 and g.ptr % 256 == 0 and g.untouched()
    g.buf[g.guard + 100] = 0
    assert not g.guards_intact()
