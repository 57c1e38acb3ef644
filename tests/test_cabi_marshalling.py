"""CPU: how _cabi.call() marshals its arguments - tensors stay referenced until the entry point has returned, None is NULL,
strided() skips the contiguity check, the argument list is checked against the signature table, and the device guard
depends on nothing but the arguments of the call at hand. The entry point is a Python stub on _cabi._lib with one
SIGNATURES entry, and the device rule is lifted through the hook tools/dry_run.py uses, so no library code runs."""
import ctypes
import weakref

import pytest
import torch

from gsplat_amd import _cabi

N = 1024


@pytest.fixture
def stub(monkeypatch):
    """stub(codes) installs gsx_stub with that signature (the stream is appended) and returns the list of argument tuples
    it was called with; CPU tensors are accepted."""
    monkeypatch.setattr(_cabi, "_refuse_host_tensor", lambda t: None)
    monkeypatch.setattr(_cabi, "current_stream", lambda: 0)

    def install(codes, on_call=None):
        seen = []

        def gsx_stub(*args):
            seen.append(args[:-1])
            if on_call is not None:
                on_call(*args[:-1])
            return 0

        monkeypatch.setitem(_cabi.SIGNATURES, "gsx_stub", ("i", list(codes) + ["p"]))
        monkeypatch.setattr(_cabi._lib, "gsx_stub", gsx_stub, raising=False)
        return seen

    return install


def _inputs():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(3, N, generator=g).t() for _ in range(3)]


def _read(addr, n):
    return torch.tensor((ctypes.c_float * n).from_address(addr)[:])


def test_temporaries_live_until_the_entry_point_returns(stub):
    """Three `.contiguous()` temporaries in one argument list: the entry point sees three distinct addresses that hold the
    three inputs' values, and the temporaries are alive while it runs and released once it has returned. The old pattern
    (data_ptr() of a dropped temporary, twice) hands out ONE address for two of them where the allocator recycles the block
    at once; whether it does depends on the heap of the process (measured: 197 of 200 tries in some processes, 0 of 200 in
    others), so the proof of life is by weak references, which holds either way, and the old pattern is only reported."""
    a, b, c = _inputs()
    assert not (a.is_contiguous() or b.is_contiguous() or c.is_contiguous())
    recycled = sum(a.contiguous().data_ptr() == b.contiguous().data_ptr() for _ in range(20))
    print(f"old pattern: the second temporary got the first one's address in {recycled} of 20 tries")
    refs, read, alive = [], [], []

    def temporaries():  # nothing but call()'s argument tuple refers to them
        for x in (a, b, c):
            t = x.contiguous()
            refs.append(weakref.ref(t))
            yield t

    def entry(*ptrs):
        alive.extend(r() is not None for r in refs)
        read.extend(_read(p, 3 * N) for p in ptrs)

    seen = stub("ppp", on_call=entry)
    _cabi.call("gsx_stub", *temporaries())
    assert alive == [True, True, True], "a temporary was released before the entry point ran"
    assert len(seen) == 1 and len(set(seen[0])) == 3, seen
    for got, want in zip(read, (a, b, c)):
        assert torch.equal(got, want.contiguous().reshape(-1))
    assert [r() for r in refs] == [None, None, None], "call() keeps its arguments after it has returned"


def test_none_strided_and_pass_through(stub):
    seen = stub("ppilfdp")
    t = torch.arange(12.0)
    view = torch.arange(24.0).reshape(12, 2)[:, 1]
    assert not view.is_contiguous()
    rec = (ctypes.c_int64 * 2)(1, 2)
    _cabi.call("gsx_stub", None, _cabi.strided(view), 3, 1 << 40, 0.5, 0.25, ctypes.addressof(rec))
    assert seen == [(None, view.data_ptr(), 3, 1 << 40, 0.5, 0.25, ctypes.addressof(rec))]
    _cabi.call("gsx_stub", t, _cabi.strided(t), 3, 4, 0.5, 0.25, rec)
    assert seen[1][:2] == (t.data_ptr(), t.data_ptr()) and seen[1][6] is rec


def test_ptr_is_a_checked_data_ptr(stub):
    t = torch.arange(24.0).reshape(12, 2)
    assert _cabi.ptr(None) is None and _cabi.ptr(t) == t.data_ptr()
    assert _cabi.ptr_strided(t[:, 1]) == t[:, 1].data_ptr()
    with pytest.raises(_cabi.GsplatAmdError, match="contiguous"):
        _cabi.ptr(t[:, 1])
    seen = stub("pp")
    _cabi.call("gsx_stub", _cabi.ptr(t), t.data_ptr())  # raw addresses still pass
    assert seen == [(t.data_ptr(), t.data_ptr())]


def test_tensor_errors(stub, monkeypatch):
    seen = stub("pp")
    t = torch.arange(24.0).reshape(12, 2)
    with pytest.raises(_cabi.GsplatAmdError, match="contiguous"):
        _cabi.call("gsx_stub", t, t[:, 1])
    monkeypatch.undo()  # the device rule is back
    with pytest.raises(_cabi.GsplatAmdError, match="no CPU fallback"):
        _cabi.ptr(t)
    with pytest.raises(_cabi.GsplatAmdError, match="no CPU fallback"):
        _cabi.ptr_strided(t)
    with pytest.raises(_cabi.GsplatAmdError, match="ROCm device.*CPU.*no CPU fallback"):
        _cabi.call("gsx_scan_i32", t, 24, t, t, 0)
    with pytest.raises(_cabi.GsplatAmdError, match="no CPU fallback"):
        _cabi.call("gsx_scan_i32", _cabi.strided(t), 24, None, None, 0)
    assert seen == []


def test_argument_list_is_checked_against_the_signature(stub):
    seen = stub("pip")
    t = torch.arange(4.0)
    for args in ((t, 1), (t, 1, t, t)):  # too few, too many
        with pytest.raises(TypeError, match="gsx_stub"):
            _cabi.call("gsx_stub", *args)
    for bad in (t, None, _cabi.strided(t)):  # only a pointer position takes these
        with pytest.raises(TypeError, match=r"gsx_stub.*argument 1\b"):
            _cabi.call("gsx_stub", t, bad, t)
    assert seen == []
    _cabi.call("gsx_stub", t, 1, None)
    assert seen == [(t.data_ptr(), 1, None)]


class _On0(torch.Tensor):
    """A host tensor that says it is on device 0."""
    is_cuda = True

    def get_device(self):
        return 0


class _On1(_On0):
    def get_device(self):
        return 1


@pytest.fixture
def guard(monkeypatch):
    """Device 0 is current; returns the list of devices that torch.cuda.device was entered with."""
    entered = []

    class device:
        def __init__(self, d):
            self.d = d

        def __enter__(self):
            entered.append(self.d)

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", device)
    return entered


def test_device_guard_follows_the_tensor_arguments(stub, guard):
    seen = stub("ppi")
    t0, t1 = torch.zeros(4).as_subclass(_On0), torch.zeros(4).as_subclass(_On1)
    _cabi.call("gsx_stub", t0, None, 1)
    assert guard == [] and len(seen) == 1  # already current
    _cabi.call("gsx_stub", t1, _cabi.strided(t1), 1)
    assert guard == [1] and len(seen) == 2
    with pytest.raises(_cabi.GsplatAmdError, match=r"gsx_stub.*cuda:0.*cuda:1"):
        _cabi.call("gsx_stub", t0, t1, 1)
    with pytest.raises(_cabi.GsplatAmdError, match=r"gsx_stub.*cuda:1.*cuda:0"):
        _cabi.call("gsx_stub", _cabi.strided(t1), t0, 1)
    assert len(seen) == 2 and len(guard) == 1


def test_a_failed_call_leaves_no_device_behind(stub, guard):
    seen = stub("ppi")
    t1 = torch.zeros(4).as_subclass(_On1)
    with pytest.raises(TypeError):
        _cabi.call("gsx_stub", t1, t1, t1)  # raises after a tensor on device 1 has been seen
    _cabi.ptr(t1)  # a pointer taken for a call that never happens
    _cabi.call("gsx_stub", 0, 0, 1)  # no tensor argument: the current device, no guard
    assert guard == [] and seen == [(0, 0, 1)]
    _cabi.call("gsx_stub", t1, None, 1)  # the observation is live: this one does enter it
    assert guard == [1]


def test_sort_pairs_goes_through_call(stub, guard, monkeypatch):
    """The flag out-parameter is an address and passes through; the guard is call()'s."""
    def set_flag(keys, vals, keys_alt, vals_alt, n, end_bit, ws, ws_bytes, flag):
        ctypes.c_int.from_address(flag).value = 1

    seen = stub("ppppliplp", on_call=set_flag)
    monkeypatch.setattr(_cabi._lib, "gsx_sort_pairs", _cabi._lib.gsx_stub)
    monkeypatch.setitem(_cabi.SIGNATURES, "gsx_sort_pairs", _cabi.SIGNATURES["gsx_stub"])
    k = torch.zeros(8, dtype=torch.int64).as_subclass(_On1)
    v = torch.zeros(8, dtype=torch.int32).as_subclass(_On1)
    ws = torch.zeros(64, dtype=torch.uint8).as_subclass(_On1)
    assert _cabi.sort_pairs(k, v, k, v, 8, 46, ws) is True
    assert seen[0][:8] == (k.data_ptr(), v.data_ptr(), k.data_ptr(), v.data_ptr(), 8, 46, ws.data_ptr(), 64)
    assert guard == [1]
