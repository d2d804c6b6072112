"""Guard-band arena: shows where a call touches memory, not only what it computes.

Every caller-owned buffer of a call is carved out of ONE uint8 buffer (an `Arena`), each at a chosen address modulo an alignment,
with a guard of at least 4096 bytes on either side (for an output: at least the bytes its 64-row x 256-column padded tile would
exceed it by, so a store that forgets a tail guard still lands inside the arena) and 1 MiB behind the last one.  `arm(pattern)`
fills the guards with a byte, the interiors of the outputs with 0xFF (NaN as fp16 / fp32, -1 as int32) and remembers the whole
arena; `verify()` then finds

  * every byte outside the outputs that changed: a store before or past an output, or into an input;
  * every output element that still holds the sentinel although its expected value does not: an element never written.

A LOAD past an input cannot be seen by looking at memory.  It is seen by running the call twice with different guard bytes
(PATTERNS: 0x00, and 0x7B -- 61280 as fp16, 1.3e36 as fp32, 123 as int8: finite and huge next to N(0, 1) data, where a NaN would
be dropped by an fmax) and comparing the outputs bit for bit (`check_footprint`): the same code on the same data may differ in
nothing but what lies next to its buffers.

Works on torch CUDA memory and on numpy (host-pointer entry points, and the CPU self-test of this module in test_footprint_cpu.py).
"""
import numpy as np

GUARD = 4096
TAIL = 1 << 20
SENTINEL = 0xFF
PATTERNS = (0x00, 0x7B)
PLACEMENTS = ((256, 0), (64, 32))       # (align, skew): a 256-byte base; ggml's tensor alignment: 32 bytes and not 64


def _np_dtype(dtype):
    """numpy dtype of a numpy / torch dtype or a name"""
    if isinstance(dtype, np.dtype):
        return dtype
    if isinstance(dtype, str) or isinstance(dtype, type):
        return np.dtype(dtype)
    name = str(dtype)                    # torch.float16 -> "float16"
    if name.startswith("torch."):
        return np.dtype(name[len("torch."):])
    return np.dtype(dtype)


def _is_numpy(buf):
    return isinstance(buf, np.ndarray)


class Arena:
    """Arena("cuda") / Arena("numpy") allocates `nbytes`; Arena(buffer) adopts a contiguous uint8 torch tensor or numpy array."""

    def __init__(self, device="cuda", nbytes=16 << 20):
        if isinstance(device, str):
            if device == "numpy":
                device = np.zeros(nbytes, np.uint8)
            else:
                import torch
                device = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.buf = device
        self.numpy = _is_numpy(device)
        assert (self.buf.dtype == np.uint8) if self.numpy else (str(self.buf.dtype) == "torch.uint8")
        assert self.buf.ndim == 1
        self.base = self.buf.ctypes.data if self.numpy else self.buf.data_ptr()
        self.size = int(self.buf.shape[0])
        self.views = []                  # dict(name, role, off, nbytes, guard, dtype, shape, view)
        self.cursor = 0                  # end of the last view's trailing guard
        self.snap = None

    # ---- layout ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def guard_bytes(shape, itemsize, role, tile=True):
        g = GUARD
        if role == "out" and tile:
            shape = tuple(int(s) for s in shape)
            cols = shape[-1] if shape else 1
            rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
            padded = -(-rows // 64) * 64 * (-(-cols // 256) * 256) * itemsize
            g = max(g, padded - rows * cols * itemsize)
        return g

    def carve(self, shape, dtype, role, align=256, skew=0, name=None, tile=True):
        """tile=False: an output that is no [N][Mw] matrix (a tap buffer of integers): the plain 4096-byte guards"""
        assert role in ("in", "out") and 0 <= skew < align
        assert self.snap is None, "carve before arm()"
        dt = _np_dtype(dtype)
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape)) * dt.itemsize
        assert skew % dt.itemsize == 0, "the view must stay aligned to its own element"
        g = self.guard_bytes(shape, dt.itemsize, role, tile)
        off = self.cursor + g
        off += (skew - (self.base + off)) % align
        end = off + nbytes
        assert end + max(g, TAIL) <= self.size, f"arena of {self.size} bytes is too small for {name or shape}"
        raw = self.buf[off:end]
        if self.numpy:
            view = raw.view(dt).reshape(shape)
        else:
            import torch
            view = raw.view(getattr(torch, dt.name)).view(shape)
        ptr = view.ctypes.data if self.numpy else view.data_ptr()
        assert ptr == self.base + off and ptr % align == skew
        self.views.append(dict(name=name or f"{role}{len(self.views)}", role=role, off=off, nbytes=nbytes, guard=g, dtype=dt, shape=shape,
                               view=view))
        self.cursor = end + g
        return view

    @property
    def used(self):
        """bytes that arm() fills and verify() looks at: everything carved, and the 1 MiB tail guard"""
        return min(self.size, (self.views[-1]["off"] + self.views[-1]["nbytes"] if self.views else 0) + TAIL)

    # ---- arm / verify ----------------------------------------------------------------------------------------------------
    def _host(self, lo, hi):
        return self.buf[lo:hi] if self.numpy else self.buf[lo:hi].cpu().numpy()

    def arm(self, pattern):
        """guards <- pattern, output interiors <- 0xFF, inputs untouched; then the snapshot verify() compares with"""
        pos = 0
        for v in self.views:
            self.buf[pos:v["off"]] = pattern
            if v["role"] == "out":
                self.buf[v["off"]:v["off"] + v["nbytes"]] = SENTINEL
            pos = v["off"] + v["nbytes"]
        self.buf[pos:self.used] = pattern
        self.pattern = pattern
        self.snap = self.buf[:self.used].copy() if self.numpy else self.buf[:self.used].clone()

    def _regions(self):
        """(lo, hi, buffer name, side, the offset the side counts from) of everything outside the output interiors, in address order"""
        out, pos, prev = [], 0, None
        for v in self.views:
            end = v["off"] + v["nbytes"]
            if prev is not None:
                mid = min(pos + prev["guard"], v["off"])
                out.append((pos, mid, prev["name"], "after", pos))
                pos = mid
            out.append((pos, v["off"], v["name"], "before", v["off"]))
            if v["role"] == "in":
                out.append((v["off"], end, v["name"], "inside (an input)", v["off"]))
            pos, prev = end, v
        if prev is not None:
            out.append((pos, self.used, prev["name"], "after", pos))
        return out

    def verify(self, expected=None):
        """expected: {name: array} of the outputs' expected values (an output not named must be written everywhere)"""
        assert self.snap is not None, "arm() first"
        if not self.numpy:
            import torch
            torch.cuda.synchronize()
        diff = self.buf[:self.used] != self.snap
        for v in self.views:
            if v["role"] == "out":
                diff[v["off"]:v["off"] + v["nbytes"]] = False
        if bool(diff.any()):
            where = np.flatnonzero(diff if self.numpy else diff.cpu().numpy())
            found = []
            for lo, hi, name, side, ref in self._regions():
                sub = where[(where >= lo) & (where < hi)]
                if sub.size:
                    found.append(f"{sub.size} byte(s) changed {side} '{name}', offsets {int(sub[0]) - ref}..{int(sub[-1]) - ref}")
            msg = "; ".join(found[:16])
            raise AssertionError(f"memory outside the outputs was written (guard pattern 0x{self.pattern:02X}): {msg}")
        for v in self.views:
            if v["role"] != "out":
                continue
            isz = v["dtype"].itemsize
            got = self._host(v["off"], v["off"] + v["nbytes"]).reshape(-1, isz)
            unwritten = (got == SENTINEL).all(axis=1)
            exp = None if expected is None else expected.get(v["name"])
            if exp is not None:
                exp = np.ascontiguousarray(exp, v["dtype"]).reshape(-1)
                assert exp.size == unwritten.size, v["name"]
                same = (exp.view(np.uint8).reshape(-1, isz) == SENTINEL).all(axis=1)      # the value itself is the sentinel's bits
                finite = np.isfinite(exp) if exp.dtype.kind == "f" else np.ones(exp.size, bool)
                unwritten &= ~same & finite
            if unwritten.any():
                idx = np.flatnonzero(unwritten)
                raise AssertionError(f"output '{v['name']}': {idx.size} element(s) never written, first {idx[0]}, last {idx[-1]}")

    def results(self):
        """{name: numpy copy} of every output"""
        if not self.numpy:
            import torch
            torch.cuda.synchronize()
        return {v["name"]: self._host(v["off"], v["off"] + v["nbytes"]).copy().view(v["dtype"]).reshape(v["shape"])
                for v in self.views if v["role"] == "out"}


class Guarded:
    """the allocation hooks a test body uses, backed by an arena at one placement and guard pattern"""

    def __init__(self, arena, align=256, skew=0, pattern=0):
        self.arena, self.align, self.skew, self.pattern = arena, align, skew, pattern

    def inp(self, data, dtype=None, name=None):
        """an input holding `data` (numpy array; converted to dtype)"""
        dt = _np_dtype(dtype) if dtype is not None else np.asarray(data).dtype
        src = np.ascontiguousarray(data, dt)
        v = self.arena.carve(src.shape, dt, "in", self.align, self.skew, name)
        if self.arena.numpy:
            v[...] = src
        else:
            import torch
            v.copy_(torch.from_numpy(src))
        return v

    def out(self, shape, dtype, name=None, tile=True):
        return self.arena.carve(shape, dtype, "out", self.align, self.skew, name, tile)

    def arm(self):
        self.arena.arm(self.pattern)

    def verify(self, expected=None):
        self.arena.verify(expected)

    def results(self):
        return self.arena.results()


PLAIN_FILL = 0xA5       # not the sentinel: an element NO run writes differs between the plain and the guarded runs, whatever its type


class Plain:
    """the same hooks on ordinary, separately allocated buffers: what every other test passes (nothing is guarded).  Outputs start as
    0xA5 bytes, so an integer element that is never written cannot pass as "the value happens to equal the sentinel"."""

    def __init__(self, device="cuda"):
        self.device, self.outs = device, []

    def inp(self, data, dtype=None, name=None):
        dt = _np_dtype(dtype) if dtype is not None else np.asarray(data).dtype
        src = np.ascontiguousarray(data, dt)
        if self.device == "numpy":
            return src.copy()
        import torch
        return torch.from_numpy(src).to(self.device)

    def out(self, shape, dtype, name=None, tile=True):
        dt = _np_dtype(dtype)
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        if self.device == "numpy":
            v = np.full(int(np.prod(shape)) * dt.itemsize, PLAIN_FILL, np.uint8).view(dt).reshape(shape)
        else:
            import torch
            v = torch.full((int(np.prod(shape)) * dt.itemsize,), PLAIN_FILL, dtype=torch.uint8, device=self.device).view(getattr(torch, dt.name)).view(shape)
        self.outs.append((name or f"out{len(self.outs)}", v))
        return v

    def arm(self):
        pass

    def verify(self, expected=None):
        pass

    def results(self):
        if self.device == "numpy":
            return {n: v.copy() for n, v in self.outs}
        import torch
        torch.cuda.synchronize()
        return {n: v.cpu().numpy() for n, v in self.outs}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_footprint(call, device="cuda", check_want=None, placements=PLACEMENTS, patterns=PATTERNS, nbytes=16 << 20):
    """The assertion every footprint case makes.  call(alloc) carves its buffers with alloc.inp / alloc.out, calls alloc.arm() right
    before the first launch and returns nothing that is not in an output.
      1. on ordinary buffers: `want` = the outputs, handed to check_want(want) (the comparison with the oracle) and finite everywhere
         (floats);
      2. at every placement and with both guard patterns, buffers carved from an armed arena: verify() holds, and every output equals
         `want` bit for bit.
    Returns want."""
    plain = Plain(device)
    call(plain)
    want = plain.results()
    for name, w in want.items():
        if w.dtype.kind == "f":
            assert np.isfinite(w).all(), f"'{name}': the unguarded run is not finite everywhere"
    if check_want is not None:
        check_want(want)
    for align, skew in placements:
        for pattern in patterns:
            g = Guarded(Arena(device, nbytes), align, skew, pattern)
            call(g)
            g.verify(want)
            got = g.results()
            assert list(got) == list(want), "the guarded run names other outputs than the plain one"
            for name, w in want.items():
                d = bits(got[name]).reshape(-1) != bits(w).reshape(-1)
                assert not d.any(), (f"'{name}' at (align {align}, skew {skew}), guard 0x{pattern:02X}: {int(d.sum())} element(s) differ from the "
                                     f"unguarded run, first {int(np.flatnonzero(d)[0])}: the result depends on the address or on neighbouring memory")
    return want
