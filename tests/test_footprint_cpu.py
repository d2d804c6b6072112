"""The guard-band harness (tests/footprint.py) must see what it claims to see: plain Python stand-ins for a kernel on a numpy arena,
one correct and five sabotaged.  No GPU, and no deliberately broken kernel, is involved."""
import numpy as np
import pytest

import footprint as fp

N_IN, N_OUT = 100, 37          # neither a multiple of any vector width


def _x():
    return np.random.default_rng(3).standard_normal(N_IN).astype(np.float16)


def _past(view, k=0):
    """the element k places past the end of a carved numpy view (k = -1 - n: before its start), through its base buffer"""
    raw = view.base if view.base is not None else view
    while raw.base is not None:
        raw = raw.base
    off = view.ctypes.data - raw.ctypes.data
    pos = off + view.nbytes + k * view.itemsize if k >= 0 else off + k * view.itemsize
    return raw[pos:pos + view.itemsize].view(view.dtype)


def good(x, y, alloc):
    y[:] = np.float32(x.astype(np.float32).sum()) + np.arange(N_OUT, dtype=np.float32)


def store_past_output(x, y, alloc):
    good(x, y, alloc)
    if isinstance(alloc, fp.Guarded):
        _past(y).view(np.uint8)[:] = 0x55


def store_before_output(x, y, alloc):
    good(x, y, alloc)
    if isinstance(alloc, fp.Guarded):
        _past(y, -1).view(np.uint8)[:] = 0x55


def store_into_input(x, y, alloc):
    good(x, y, alloc)
    x[N_IN - 1] = 0


def element_unwritten(x, y, alloc):
    keep = y[N_OUT - 1].copy()
    good(x, y, alloc)
    if isinstance(alloc, fp.Guarded):
        y[N_OUT - 1] = keep


def load_past_input(x, y, alloc):
    """an abs-max that walks one element too far.  (Like the other stand-ins it misbehaves in the guarded runs only: it models "on
    ordinary buffers the neighbour happened not to matter", the case the existing suite cannot see, not a neighbour read in the plain run.)"""
    good(x, y, alloc)
    if isinstance(alloc, fp.Guarded):
        y[0] += np.float32(max(np.abs(x.astype(np.float32)).max(), abs(np.float32(_past(x)[0]))))
    else:
        y[0] += np.float32(np.abs(x.astype(np.float32)).max())


def run(kernel, device="numpy"):
    def call(alloc):
        x = alloc.inp(_x(), name="x")
        y = alloc.out((N_OUT,), np.float32, name="y")
        alloc.arm()
        kernel(x, y, alloc)
    return fp.check_footprint(call, device=device, nbytes=4 << 20)


def test_correct_stand_in_passes():
    want = run(good)
    assert np.array_equal(want["y"], np.float32(_x().astype(np.float32).sum()) + np.arange(N_OUT, dtype=np.float32))


@pytest.mark.parametrize("kernel,message", [
    (store_past_output, r"changed after 'y', offsets 0\.\.3"),
    (store_before_output, r"changed before 'y', offsets -4\.\.-1"),
    (store_into_input, r"changed inside \(an input\) 'x', offsets 198\.\.199"),
    (element_unwritten, r"output 'y': 1 element\(s\) never written, first 36, last 36"),
    (load_past_input, r"'y' at \(align 256, skew 0\), guard 0x7B: 1 element\(s\) differ"),
], ids=lambda v: v.__name__ if callable(v) else "")
def test_sabotaged_stand_ins_are_caught(kernel, message):
    with pytest.raises(AssertionError, match=message):
        run(kernel)


def test_integer_element_that_no_run_writes_is_caught():
    """an int32 output whose last element neither the plain nor the guarded runs write: the plain run's 0xA5 fill is not the sentinel, so
    the guarded run cannot pass it off as a value of -1"""
    def call(alloc):
        t = alloc.out((N_OUT,), np.int32, name="tap", tile=False)
        alloc.arm()
        t[:N_OUT - 1] = np.arange(N_OUT - 1)

    with pytest.raises(AssertionError, match=r"output 'tap': 1 element\(s\) never written, first 36, last 36"):
        fp.check_footprint(call, device="numpy", nbytes=4 << 20)


def test_layout():
    """every view starts at skew modulo align, guards of at least 4096 bytes (an output: at least its padded tile's excess), a 1 MiB
    tail, and arm() leaves the inputs alone"""
    a = fp.Arena("numpy", 8 << 20)
    x = a.carve((100,), np.float16, "in", 64, 32, "x")
    y = a.carve((70, 320), np.float32, "out", 64, 32, "y")
    t = a.carve((5,), np.int32, "out", 256, 0, "t")
    x[:] = 1
    for v in (x, y):
        assert v.ctypes.data % 64 == 32
    assert t.ctypes.data % 256 == 0
    vx, vy, vt = a.views
    assert vy["guard"] == 128 * 512 * 4 - 70 * 320 * 4 and vx["guard"] == fp.GUARD and vt["guard"] == 64 * 256 * 4 - 5 * 4
    assert vy["off"] - (vx["off"] + vx["nbytes"]) >= vx["guard"] + vy["guard"]
    assert vt["off"] - (vy["off"] + vy["nbytes"]) >= vy["guard"] + vt["guard"]
    assert a.used == vt["off"] + vt["nbytes"] + fp.TAIL <= a.size
    a.arm(0x7B)
    assert (x == 1).all() and np.isnan(y).all() and (t == -1).all()
    assert (a.buf[:vx["off"]] == 0x7B).all() and (a.buf[vt["off"] + vt["nbytes"]:a.used] == 0x7B).all()
    with pytest.raises(AssertionError, match="never written"):
        a.verify()
    y[:] = 0; t[:] = -1
    a.verify({"t": np.full(5, -1, np.int32)})            # -1 is the expected tap value there: written
    with pytest.raises(AssertionError, match="'t'"):
        a.verify()
    a.buf[a.used - 1] = 0
    with pytest.raises(AssertionError, match=r"changed after 't'"):
        a.verify({"t": np.full(5, -1, np.int32)})
