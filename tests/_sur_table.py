"""Table-level harness for the kernels of spmf_amd/csrc/surrogate.hip -- TEST INFRASTRUCTURE ONLY.

Drives the C-ABI entry points (spmf_surrogate_fwd / _bwd / _bwd_adam_dev, spmf_adam_step / _dev,
spmf_vi_gate, spmf_sample_noise / _transform) over raw torch buffers with any context handle, so n, kind,
ident, noise_ld, S and the slot layout are free.  Two things keep a mistake here from becoming an
out-of-bounds write on the device:

  * every buffer is checked on the host (dtype, contiguity, element count against n, S, noise_ld)
    before a call; a mismatch raises and nothing is launched;
  * every output / in-place buffer lives inside a larger allocation with MARGIN sentinel elements on
    both sides (Guarded); after every call the margins must be bit-identical.  A kernel that writes
    past n at a block edge is caught without the write leaving the allocation.

The grids of the edge tests (gamma_grid, normal_slot_inputs, ...) are here too: they need numpy only, so the host
suite can count what the fp32 range leaves out.
"""
import numpy as np
import torch

from spmf_amd import _lib

import _sur_reference as R

MARGIN = 64
_SENT = {torch.float32: (torch.int32, 0x7FA5C3E1), torch.float64: (torch.int64, 0x7FF5A5C3E1D2B4A6),
         torch.uint8: (torch.uint8, 0xA5)}
#: second pattern: the columns of a wide noise buffer that belong to no slot (noise_ld > n)
_GAP = 0x7FB6D4F2


class Guarded:
    """`count` elements of `dtype` with MARGIN sentinel elements before and after; `shift` moves the body
    that many elements further in (shift = 1: a float32 body that is 4-byte but not 16-byte aligned)."""

    def __init__(self, count, dtype=torch.float32, device="cuda", shift=0, fill=None):
        self.count, self.dtype, self.lo = int(count), dtype, MARGIN + int(shift)
        self.buf = torch.empty(self.lo + self.count + MARGIN, dtype=dtype, device=device)
        idt, pat = _SENT[dtype]
        self.buf.view(idt).fill_(pat)
        self.t = self.buf[self.lo:self.lo + self.count]
        if fill is not None:
            self.set(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def set(self, a):
        a = torch.as_tensor(np.ascontiguousarray(a)).reshape(-1)
        if a.numel() != self.count:
            raise ValueError(f"Guarded.set: {a.numel()} elements for a body of {self.count}")
        self.t.copy_(a.to(self.dtype))
        return self

    def get(self):
        return self.t.detach().cpu().numpy().copy()

    def bits(self):
        return self.t.view(_SENT[self.dtype][0]).clone()

    def intact(self):
        idt, pat = _SENT[self.dtype]
        b = self.buf.view(idt)
        return bool((b[:self.lo] == pat).all()) and bool((b[self.lo + self.count:] == pat).all())


def _need(t, dtype, count, what):
    """The host-side check of one buffer handed to the library."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: not a device tensor")
    if t.dtype != dtype:
        raise ValueError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    if t.numel() != count:
        raise ValueError(f"{what}: {t.numel()} elements, expected {count}")


class SurSlot:
    """One variable of a table.  noise / dgda: [S, n] host arrays (or None: left as sentinels, for the sampler
    to fill); ld > n places them as a column slice of a [S, ld] buffer, as Surrogate.alloc_noise does."""

    def __init__(self, S, n, kind, t0, t1, noise=None, dgda=None, gtheta=None, ident=None, ld=None,
                 device="cuda", big=False):
        self.S, self.n, self.kind = int(S), int(n), int(kind)
        self.ld = self.n if ld is None else int(ld)
        if self.ld < self.n:
            raise ValueError("noise_ld < n")
        self.off = (self.ld - self.n) // 2
        self.t0 = Guarded(n, fill=t0, device=device)
        self.t1 = Guarded(n, fill=t1, device=device)
        self.noise_w = Guarded(self.S * self.ld, device=device)
        self.dgda_w = Guarded(self.S * self.ld, device=device) if kind == 2 else None
        for w, a in ((self.noise_w, noise), (self.dgda_w, dgda)):
            if w is None:
                continue
            if self.ld > self.n:
                w.t.view(torch.int32).fill_(_GAP)
            if a is not None:
                self._cols(w).copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).reshape(self.S, self.n))
        self.theta = Guarded(self.S * self.n, device=device)
        self.gtheta = None if gtheta is None else Guarded(self.S * self.n, fill=gtheta, device=device)
        self.g0 = None if big else Guarded(n, device=device)
        self.g1 = None if big else Guarded(n, device=device)
        self.ident = None if ident is None else Guarded(n, torch.uint8, fill=np.asarray(ident, dtype=np.uint8),
                                                        device=device)
        self.m = self.v = None         # Adam records of t0 / t1 (pairs), set by SurTable.attach_adam

    def _cols(self, w):
        return w.t.view(self.S, self.ld)[:, self.off:self.off + self.n]

    def noise(self):
        return self._cols(self.noise_w).detach().cpu().numpy().copy()

    def dgda(self):
        return self._cols(self.dgda_w).detach().cpu().numpy().copy()

    def noise_ptr(self, w):
        return w.ptr + 4 * self.off

    def guarded(self):
        g = [self.t0, self.t1, self.noise_w, self.dgda_w, self.theta, self.gtheta, self.g0, self.g1, self.ident]
        if self.m is not None:
            g += list(self.m) + list(self.v)
        return [x for x in g if x is not None]

    def gaps_intact(self):
        if self.ld == self.n:
            return True
        for w in (self.noise_w, self.dgda_w):
            if w is None:
                continue
            b = w.t.view(torch.int32).view(self.S, self.ld)
            if not bool((b[:, :self.off] == _GAP).all()) or not bool((b[:, self.off + self.n:] == _GAP).all()):
                return False
        return True

    def validate(self, need):
        _need(self.t0.t, torch.float32, self.n, "t0")
        _need(self.t1.t, torch.float32, self.n, "t1")
        if self.n < 1 or self.kind not in (0, 1, 2):
            raise ValueError("bad n / kind")
        # the kernels touch noise[s * ld + i], i < n, from the slot's pointer: the last one must be inside
        last = self.off + (self.S - 1) * self.ld + self.n
        for w, nm in ((self.noise_w, "noise"), (self.dgda_w, "dgda")):
            if w is not None:
                _need(w.t, torch.float32, self.S * self.ld, nm)
                if last > w.count:
                    raise ValueError(f"{nm}: the slice ends at {last} of {w.count}")
        if self.kind == 2 and self.dgda_w is None:
            raise ValueError("kind 2 without dgda")
        _need(self.theta.t, torch.float32, self.S * self.n, "theta")
        if "gtheta" in need:
            if self.gtheta is None:
                raise ValueError("gtheta missing")
            _need(self.gtheta.t, torch.float32, self.S * self.n, "gtheta")
        if "g01" in need:
            if self.g0 is None or self.g1 is None:
                raise ValueError("g0 / g1 missing")
            _need(self.g0.t, torch.float32, self.n, "g0")
            _need(self.g1.t, torch.float32, self.n, "g1")
        if "adam" in need:
            if self.m is None:
                raise ValueError("Adam records missing")
            for x in list(self.m) + list(self.v):
                _need(x.t, torch.float32, self.n, "adam m / v")
        if self.ident is not None:
            _need(self.ident.t, torch.uint8, self.n, "ident")


class SurTable:
    """slots: list of SurSlot or None (a skipped variable, n = 0)."""

    def __init__(self, handle, S, slots, device="cuda"):
        if not 1 <= len(slots) <= _lib.NVARS:
            raise ValueError("1..12 variables")
        if not 1 <= S <= 65535:
            raise ValueError("S out of range")
        self.h, self.S, self.slots, self.device = handle, int(S), list(slots), device
        for sl in self.slots:
            if sl is not None and sl.S != self.S:
                raise ValueError("slot built for another S")
        self.logq = Guarded(self.S, torch.float64, device=device)
        self.lib = _lib.load()

    def _arr(self, need, allow_skip, skip=()):
        """The ctypes table after the host-side checks; `skip`: indices handed over as n = 0 although the
        slot has buffers (they must come back untouched)."""
        arr = (_lib.SurVar * len(self.slots))()
        for i, sl in enumerate(self.slots):
            if sl is None or i in skip:
                if not allow_skip:
                    raise ValueError("this entry point takes no skipped variable")
                arr[i].n = 0
                continue
            sl.validate(need)
            v = arr[i]
            v.t0, v.t1, v.n, v.kind = sl.t0.ptr, sl.t1.ptr, sl.n, sl.kind
            v.noise, v.noise_ld = sl.noise_ptr(sl.noise_w), (sl.ld if sl.ld != sl.n else 0)
            v.dgda = sl.noise_ptr(sl.dgda_w) if sl.dgda_w is not None else None
            v.theta = sl.theta.ptr
            v.gtheta = sl.gtheta.ptr if sl.gtheta is not None else None
            v.g0 = sl.g0.ptr if sl.g0 is not None else None
            v.g1 = sl.g1.ptr if sl.g1 is not None else None
            v.ident = sl.ident.ptr if sl.ident is not None else None
        if all(sl is None or i in skip for i, sl in enumerate(self.slots)):
            raise ValueError("every variable skipped")
        _need(self.logq.t, torch.float64, self.S, "logq")
        return arr

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _done(self, what):
        torch.cuda.synchronize()
        bad = [what for g in [self.logq] + [g for sl in self.slots if sl is not None for g in sl.guarded()]
               if not g.intact()]
        assert not bad, f"{what}: a canary margin was written"
        assert all(sl.gaps_intact() for sl in self.slots if sl is not None), \
            f"{what}: a column outside the slot's slice of the wide noise buffer was written"

    def fwd(self, skip=()):
        arr = self._arr((), True, skip)
        _lib.check(self.h, self.lib.spmf_surrogate_fwd(self.h, arr, len(self.slots), self.S, self.logq.ptr,
                                                       self._stream()), "spmf_surrogate_fwd")
        self._done("spmf_surrogate_fwd")

    def bwd(self, inv_sb, c):
        arr = self._arr(("gtheta", "g01"), False)
        _lib.check(self.h, self.lib.spmf_surrogate_bwd(self.h, arr, len(self.slots), self.S, float(inv_sb),
                                                       float(c), self._stream()), "spmf_surrogate_bwd")
        self._done("spmf_surrogate_bwd")

    def attach_adam(self, rng):
        """Adam records (m, v) for t0 / t1 of every slot, random m and positive v; -> nothing."""
        for sl in self.slots:
            sl.m = tuple(Guarded(sl.n, fill=rng.normal(0, 1e-2, sl.n), device=self.device) for _ in range(2))
            sl.v = tuple(Guarded(sl.n, fill=rng.uniform(1e-6, 1e-2, sl.n), device=self.device) for _ in range(2))

    def bwd_adam(self, inv_sb, c, state):
        arr = self._arr(("gtheta", "adam"), False)
        _need(state, torch.float64, _lib.VI_STATE_LEN, "state")
        av = (_lib.AdamVar * (2 * len(self.slots)))()
        for i, sl in enumerate(self.slots):
            for j, p in enumerate((sl.t0, sl.t1)):
                a = av[2 * i + j]
                a.p, a.m, a.v, a.g, a.n = p.ptr, sl.m[j].ptr, sl.v[j].ptr, None, sl.n
        _lib.check(self.h, self.lib.spmf_surrogate_bwd_adam_dev(
            self.h, arr, len(self.slots), self.S, float(inv_sb), float(c), av, state.data_ptr(), self._stream()),
            "spmf_surrogate_bwd_adam_dev")
        self._done("spmf_surrogate_bwd_adam_dev")

    def sample_noise(self, seed, counter=0, state=None, skip=()):
        arr = self._arr((), True, skip)
        if state is not None:
            _need(state, torch.float64, _lib.VI_STATE_LEN, "state")
        _lib.check(self.h, self.lib.spmf_sample_noise(self.h, arr, len(self.slots), self.S, int(seed), int(counter),
                                                      state.data_ptr() if state is not None else None,
                                                      self._stream()), "spmf_sample_noise")
        self._done("spmf_sample_noise")

    def sample_transform(self, seed, counter=0, state=None, skip=()):
        arr = self._arr((), True, skip)
        if state is not None:
            _need(state, torch.float64, _lib.VI_STATE_LEN, "state")
        _lib.check(self.h, self.lib.spmf_sample_transform(
            self.h, arr, len(self.slots), self.S, int(seed), int(counter),
            state.data_ptr() if state is not None else None, self.logq.ptr, self._stream()), "spmf_sample_transform")
        self._done("spmf_sample_transform")


class AdamTable:
    """tensors: list of dict(n, p, m, v, g, shift=(sp, sm, sv, sg)): shift 1 starts that array one element
    into its buffer (4-byte aligned only: the scalar branch of adam_block)."""

    def __init__(self, handle, tensors, device="cuda"):
        if not 1 <= len(tensors) <= 24:
            raise ValueError("1..24 tensors")
        self.h, self.device, self.lib = handle, device, _lib.load()
        self.rec = []
        for t in tensors:
            sh = t.get("shift", (0, 0, 0, 0))
            self.rec.append({k: Guarded(t["n"], fill=t[k], shift=s, device=device)
                             for k, s in zip("pmvg", sh)} | {"n": int(t["n"])})

    def _arr(self):
        arr = (_lib.AdamVar * len(self.rec))()
        for a, r in zip(arr, self.rec):
            if r["n"] < 1:
                raise ValueError("n < 1")
            for k in "pmvg":
                _need(r[k].t, torch.float32, r["n"], k)
                if r[k].ptr % 4:
                    raise ValueError("unaligned float")
            a.p, a.m, a.v, a.g, a.n = r["p"].ptr, r["m"].ptr, r["v"].ptr, r["g"].ptr, r["n"]
        return arr

    def _done(self, what):
        torch.cuda.synchronize()
        assert all(r[k].intact() for r in self.rec for k in "pmvg"), f"{what}: a canary margin was written"

    def step(self, lr, b1, b2, eps, t, clip):
        arr = self._arr()
        if t < 1:
            raise ValueError("step is 1-based")
        _lib.check(self.h, self.lib.spmf_adam_step(self.h, arr, len(self.rec), float(lr), float(b1), float(b2),
                                                   float(eps), int(t), float(clip),
                                                   torch.cuda.current_stream(self.device).cuda_stream),
                   "spmf_adam_step")
        self._done("spmf_adam_step")

    def step_dev(self, state):
        arr = self._arr()
        _need(state, torch.float64, _lib.VI_STATE_LEN, "state")
        _lib.check(self.h, self.lib.spmf_adam_step_dev(self.h, arr, len(self.rec), state.data_ptr(),
                                                       torch.cuda.current_stream(self.device).cuda_stream),
                   "spmf_adam_step_dev")
        self._done("spmf_adam_step_dev")

    def host(self, k):
        return [r[k].get() for r in self.rec]


def vi_gate(handle, state, parts, logq, nnf, S, c, rows):
    """spmf_vi_gate on a Guarded state (in place); parts [S,14], logq [S], nnf [2S] or None: device fp64."""
    _need(state.t, torch.float64, _lib.VI_STATE_LEN, "state")
    _need(parts, torch.float64, 14 * S, "parts")
    _need(logq, torch.float64, S, "logq")
    if nnf is not None:
        _need(nnf, torch.float64, 2 * S, "n_nonfinite")
    lib = _lib.load()
    _lib.check(handle, lib.spmf_vi_gate(handle, parts.data_ptr(), logq.data_ptr(),
                                        nnf.data_ptr() if nnf is not None else None, int(S), float(c), float(rows),
                                        state.ptr, torch.cuda.current_stream().cuda_stream), "spmf_vi_gate")
    torch.cuda.synchronize()
    assert state.intact(), "spmf_vi_gate: a canary margin was written"


# ---- the grids of the edge tests (numpy only) --------------------------------------------------

GAMMA_A = (1e-3, 0.05, 0.1, 0.3, float(np.nextafter(np.float32(1), np.float32(0))),
           float(np.nextafter(np.float32(1), np.float32(2))), 3.0, 50.0, 300.0)
GAMMA_B = (7e-3, 1.0, 20.0, 1e6, 2e10)
GAMMA_G = (1e-30, 1e-25, 1e-20, 1e-6, 0.1, 1.0, 10.0, 1e3)
FP32_RANGE = 1e37
GTHETA_MAX = 1e6


def raw_of(x):
    """fp32 raw trainable whose softplus is (to fp32 rounding) x."""
    return np.float32(R.softplus_inv(x))


def gamma_dgda(a, g):
    """The dgda handed to the chain-rule kernels at (a, g): dgda_ref where mpmath is cheap (moderate g),
    the small-g leading term below 1e-3 -- any finite value of the right magnitude serves, the kernels
    are handed it."""
    if g < 1e-3:
        return float(R.dgda_small(a, g))
    return R.dgda_ref(float(a), float(g), 40)


def gamma_grid(inv_sb, c):
    """The kind-2 grid (a, b, g) with its hand-set dgda, and which combinations stay: one is left out when
    its fp64 reference leaves the fp32 range -- |y|, theta, or either gradient at gtheta in {0, +-1e6},
    above 1e37.
    -> list of (t0, t1, g, dgda, keep); t0 / t1 are the fp32 raw values, a is softplus(t0) in fp64."""
    out = []
    for a0 in GAMMA_A:
        t0 = raw_of(a0)
        a = float(R.softplus(np.float64(t0)))
        for b0 in GAMMA_B:
            t1 = raw_of(b0)
            for g in GAMMA_G:
                g32 = np.float32(g)
                dg = np.float32(gamma_dgda(a, float(g32)))
                f = R.fwd_ref(2, [t0], [t1], [[g32]])
                grad = 0.0
                for ge in (0.0, GTHETA_MAX, -GTHETA_MAX):
                    g0, g1, _, _ = R.bwd_ref(2, [t0], [t1], [[g32]], [[ge]], inv_sb, c, [[dg]])
                    grad = max(grad, abs(g0[0]), abs(g1[0]))
                keep = (np.isfinite(dg) and abs(f["y"][0, 0]) < FP32_RANGE and f["theta"][0, 0] < FP32_RANGE
                        and grad < FP32_RANGE)
                out.append((t0, t1, g32, dg, bool(keep)))
    return out


NORMAL_T1 = (-20.0, -7.6, 0.0, 5.0, 20.0)
NORMAL_EPS = tuple(np.linspace(-6.0, 6.0, 13))          # holds the exact 0


def normal_slot_inputs(n, S, rng):
    """t0 in [-30, 30] (both ends and 0 included), raw scale from NORMAL_T1, eps from NORMAL_EPS."""
    t0 = rng.uniform(-30.0, 30.0, n).astype(np.float32)
    t0[:3] = (-30.0, 30.0, 0.0)[:min(n, 3)]
    t1 = np.asarray(NORMAL_T1, dtype=np.float32)[(np.arange(n) + rng.integers(5)) % 5]
    e = np.asarray(NORMAL_EPS, dtype=np.float32)
    eps = e[(np.arange(n)[None, :] // 5 + 4 * np.arange(S)[:, None] + rng.integers(13)) % 13]
    return t0, t1, eps


def gamma_slot_inputs(n, S, grid, rng):
    """n elements over the 45 (a, b) pairs of the grid; draw s of element i takes the next g of GAMMA_G whose
    combination stays (see gamma_grid)."""
    ng, npair = len(GAMMA_G), len(GAMMA_A) * len(GAMMA_B)
    pair = (np.arange(n) + rng.integers(npair)) % npair
    t0 = np.array([grid[p * ng][0] for p in pair], dtype=np.float32)
    t1 = np.array([grid[p * ng][1] for p in pair], dtype=np.float32)
    g = np.empty((S, n), dtype=np.float32)
    dg = np.empty((S, n), dtype=np.float32)
    start = rng.integers(ng)
    for s in range(S):
        for i in range(n):
            k = (i // npair + 3 * s + start) % ng
            for _ in range(ng):
                if grid[pair[i] * ng + k][4]:
                    break
                k = (k + 1) % ng
            g[s, i], dg[s, i] = grid[pair[i] * ng + k][2], grid[pair[i] * ng + k][3]
    return t0, t1, g, dg


def gtheta_inputs(S, n, rng):
    """dE/dtheta: random over twelve decades up to 1e6, both signs, one entry in five exactly 0."""
    ge = rng.normal(0, 1, (S, n)) * 10.0 ** rng.uniform(-6, 6, (S, n))
    ge = np.clip(ge, -GTHETA_MAX, GTHETA_MAX)
    ge[rng.random((S, n)) < 0.2] = 0.0
    if n >= 2:
        ge[0, 0], ge[-1, -1] = GTHETA_MAX, -GTHETA_MAX
    return ge.astype(np.float32)
