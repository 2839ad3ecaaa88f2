"""The model elementwise and max-pool kernels (wam_amd/csrc/model_ew.hip) at the C ABI against the
plain-numpy references of tests/modelew_ref.py, one entry at a time, and the Python wrappers of
wam_amd/model_fuse.py against the same expressions in torch float64.

Comparison: the contract is a fixed sequence of fp32 adds, a compare and one rounding on the store,
without a multiply, so every kernel result has to EQUAL the reference -- NaN exactly where the
reference has NaN, zeros by value (the sign of a zero is not part of the contract), everything
else bit for bit. There is no tolerance anywhere in this file.

Every output lives inside a larger device buffer with PAD sentinel elements on both sides, which
must be intact afterwards; inputs sit PAD elements away from the ends of their allocations too.
Operands are `off` elements past a 16-byte boundary where a case asks for a misaligned pointer.

Routes (channel_layout in model_ew.hip; V = 4 fp32 / 8 bf16 elements per 16-byte vector): `route`
below restates the selection, and every row of the case tables is asserted to take the route
written next to it.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import modelew_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 64                      # guard elements: 256 / 128 bytes, so the payload stays 16-byte aligned
OK, INVALID, UNSUPPORTED = 0, 1, 3
SENTINEL = {False: np.array([-12345.0], dtype=F32).view(np.uint32)[0], True: np.uint16(0xC641)}
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
FLT_MAX = float(np.finfo(F32).max)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, BF16_MAX, 2.0 ** 119, 1.0, 1.0078125, 2.0 ** -8,
                     -1.0, -1.0078125, -2.0 ** -8, FLT_MAX], dtype=F32)
# (p, q) placed at the same index of two operands that are added:
PAIRS = [(BF16_MAX, 2.0 ** 119),      # (2 - 2^-8) 2^127: finite in fp32, the tie that rounds to bf16 infinity
         (1.0, 2.0 ** -8),            # bf16 tie, last bit even: rounds down to 1
         (1.0078125, 2.0 ** -8),      # bf16 tie, last bit odd: rounds up to 1 + 2^-6
         (-1.0078125, -2.0 ** -8),    # the same below zero (kept by bias_act with relu = 0)
         (FLT_MAX, FLT_MAX),          # overflows in fp32 itself (bf16 storage holds infinity already)
         (-1.0, -2.0 ** -8), (np.inf, -np.inf), (-0.0, -0.0), (-0.0, 0.0), (np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (-np.inf, 1.0)]


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def V_of(bf16):
    return 8 if bf16 else 4


class Buf:
    """n elements of the storage type in the middle of a sentinel-filled device buffer, `off`
    elements past a 16-byte boundary. vals: float32 values, rounded to the storage type on the way
    in (`.vals` is what the kernel reads); None: the payload holds the sentinel as well."""

    def __init__(self, bf16, n, vals=None, off=0):
        self.bf16, self.n, self.lo = bf16, n, PAD + off
        self.host = np.full(PAD + off + n + PAD, SENTINEL[bf16], dtype=np.uint16 if bf16 else np.uint32)
        self.vals = None
        if vals is not None:
            vals = np.asarray(vals, dtype=F32)
            assert vals.shape == (n,)
            self.vals = R.store(vals, bf16)
            self.host[self.lo:self.lo + n] = R.f32_to_bf16(vals) if bf16 else vals.view(np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int16 if bf16 else np.int32).copy()).cuda()
        self.addr = self.dev.data_ptr() + self.lo * self.host.itemsize
        assert self.dev.data_ptr() % 16 == 0 and (self.addr % 16 == 0) == (off * self.host.itemsize % 16 == 0)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def read(self, what):
        """payload as float32 values, after checking that both guards still hold the sentinel"""
        raw = self.dev.cpu().numpy().view(self.host.dtype)
        assert (raw[:self.lo] == SENTINEL[self.bf16]).all(), "%s: the guard below the output was written" % what
        assert (raw[self.lo + self.n:] == SENTINEL[self.bf16]).all(), "%s: the guard above the output was written" % what
        pay = raw[self.lo:self.lo + self.n]
        return R.bf16_to_f32(pay) if self.bf16 else pay.view(F32).copy()

    def untouched(self):
        return bool((self.dev.cpu().numpy().view(self.host.dtype) == SENTINEL[self.bf16]).all())


def values(rng, n, bf16):
    return R.store((rng.standard_normal(n) * 2.0).astype(F32), bf16)


def P(b):
    return None if b is None else b.ptr


def stream(L):
    return L.stream_of(torch.device("cuda"))


def check_out(buf, ref, what):
    R.assert_same(buf.read(what), R.store(ref, buf.bf16), what)


# ------------------------------------------------------------------------------ elementwise routes
def route(V, n, C, inner, ptr_offs, bias_offs, itemsize):
    """channel_layout restated: the kernel a call runs"""
    if n % V or any(o * itemsize % 16 for o in ptr_offs):
        return "scalar"
    if inner == 1 and C % V == 0:
        return "scalar" if any(o * itemsize % 16 for o in bias_offs) else "CH_VEC"
    return "CH_ONE" if inner % V == 0 else "scalar"


def ew_cases(V):
    """(name, n, C, inner, misaligned operand or None, route, the condition that selects it)"""
    return [
        ("vec", 21 * V, 3 * V, 1, None, "CH_VEC", "inner == 1, C % V == 0, n % V == 0, all aligned"),
        ("one", 30 * V, 5, 2 * V, None, "CH_ONE", "inner % V == 0 (C = 5 is no multiple of V)"),
        ("ragged", 21 * V + 3, 3 * V, 1, None, "scalar", "n % V != 0"),
        ("halfvec", 6 * V, V + V // 2, 1, None, "scalar", "inner == 1 but C % V != 0 (and inner % V != 0)"),
        ("inner49", 1960, 5, 49, None, "scalar", "inner = 49: neither inner == 1 nor inner % V == 0"),
        ("vec_off_0", 21 * V, 3 * V, 1, 0, "scalar", "first operand (a / y of bias_act / g1) one element off 16 bytes"),
        ("vec_off_1", 21 * V, 3 * V, 1, 1, "scalar", "second operand (s / g2) one element off"),
        ("vec_off_2", 21 * V, 3 * V, 1, 2, "scalar", "third operand (out of add_bias_relu / y of relu_mask) one element off"),
        ("vec_off_3", 21 * V, 3 * V, 1, 3, "scalar", "fourth operand (out of relu_mask) one element off"),
        ("one_off_0", 30 * V, 5, 2 * V, 0, "scalar", "CH_ONE shape, first operand one element off"),
        ("vec_bias_a_off", 21 * V, 3 * V, 1, "ba", "scalar", "CH_VEC shape, first bias one element off (16-byte bias loads)"),
        ("vec_bias_s_off", 21 * V, 3 * V, 1, "bs", "scalar", "CH_VEC shape, second bias one element off"),
        ("one_bias_a_off", 30 * V, 5, 2 * V, "ba", "CH_ONE", "CH_ONE reads its bias one element at a time: stays vectorised"),
    ]


CASE_NAMES = [c[0] for c in ew_cases(4)]


def _case(bf16, name):
    return next(c for c in ew_cases(V_of(bf16)) if c[0] == name)


def run_add_bias_relu(L, bf16, n, C, inner, rng, use=(True, True), mis=None, alias=None, a=None, s=None, ba=None,
                      bs=None, what=""):
    V = V_of(bf16)
    off = lambda i: 1 if mis == i else 0  # noqa: E731
    A = Buf(bf16, n, values(rng, n, bf16) if a is None else a, off(0))
    S = Buf(bf16, n, values(rng, n, bf16) if s is None else s, off(1))
    BA = Buf(bf16, C, values(rng, C, bf16) if ba is None else ba, 1 if mis == "ba" else 0) if use[0] else None
    BS = Buf(bf16, C, values(rng, C, bf16) if bs is None else bs, 1 if mis == "bs" else 0) if use[1] else None
    O = {"a": A, "s": S, None: None}[alias] or Buf(bf16, n, None, off(2))
    offs = [A.lo - PAD, S.lo - PAD, O.lo - PAD]
    r = route(V, n, C, inner, offs, [b.lo - PAD for b in (BA, BS) if b is not None], A.host.itemsize)
    rc = L.lib.wam_ew_add_bias_relu(int(bf16), n, C, inner, A.ptr, P(BA), S.ptr, P(BS), O.ptr, stream(L))
    torch.cuda.synchronize()
    assert rc == OK, what
    ref = R.add_bias_relu_ref(A.vals, BA and BA.vals, S.vals, BS and BS.vals, C, inner)
    check_out(O, ref, "add_bias_relu %s %s bias=%s alias=%s [%s]" % ("bf16" if bf16 else "fp32", what, use, alias, r))
    for b in (A, S):  # the inputs are read only
        if b is not O:
            R.assert_same(b.read(what), b.vals, "add_bias_relu input " + what)
    return r


def run_bias_act(L, bf16, n, C, inner, rng, use=True, relu=1, mis=None, y=None, b=None, what=""):
    V = V_of(bf16)
    Y = Buf(bf16, n, values(rng, n, bf16) if y is None else y, 1 if mis == 0 else 0)
    B = Buf(bf16, C, values(rng, C, bf16) if b is None else b, 1 if mis == "ba" else 0) if use else None
    r = route(V, n, C, inner, [Y.lo - PAD], [B.lo - PAD] if B is not None else [], Y.host.itemsize)
    rc = L.lib.wam_ew_bias_act(int(bf16), n, C, inner, Y.ptr, P(B), relu, stream(L))
    torch.cuda.synchronize()
    assert rc == OK, what
    ref = R.bias_act_ref(Y.vals, B and B.vals, C, inner, relu)
    check_out(Y, ref, "bias_act %s %s bias=%s relu=%d [%s]" % ("bf16" if bf16 else "fp32", what, use, relu, r))
    return r


def run_relu_mask(L, bf16, n, rng, two=True, mis=None, alias=None, g1=None, g2=None, y=None, what=""):
    V = V_of(bf16)
    off = lambda i: 1 if mis == i else 0  # noqa: E731
    G1 = Buf(bf16, n, values(rng, n, bf16) if g1 is None else g1, off(0))
    G2 = Buf(bf16, n, values(rng, n, bf16) if g2 is None else g2, off(1)) if two else None
    if y is None:  # a ReLU output: half zeros, some -0.0
        y = np.maximum(values(rng, n, bf16), 0)
        y[rng.uniform(size=n) < 0.1] = -0.0
    Y = Buf(bf16, n, y, off(2))
    O = {"g1": G1, "g2": G2, "y": Y, None: None}[alias] or Buf(bf16, n, None, off(3))
    offs = [b.lo - PAD for b in (G1, G2, Y, O) if b is not None]
    r = route(V, n, V, 1, offs, [], G1.host.itemsize)
    rc = L.lib.wam_ew_relu_mask(int(bf16), n, G1.ptr, P(G2), Y.ptr, O.ptr, stream(L))
    torch.cuda.synchronize()
    assert rc == OK, what
    ref = R.relu_mask_ref(G1.vals, G2 and G2.vals, Y.vals)
    check_out(O, ref, "relu_mask %s %s g2=%s alias=%s [%s]" % ("bf16" if bf16 else "fp32", what, two, alias, r))
    for b in (G1, G2, Y):
        if b is not None and b is not O:
            R.assert_same(b.read(what), b.vals, "relu_mask input " + what)
    return "vec" if r == "CH_VEC" else r


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", [c for c in CASE_NAMES if c != "vec_off_3"])  # three tensor operands
def test_add_bias_relu_routes(L, name, bf16):
    """wam_ew_add_bias_relu on every row of the route table: both, either and no bias; out a buffer
    of its own, out == a and out == s."""
    _, n, C, inner, mis, want, _ = _case(bf16, name)
    rng = np.random.RandomState(len(name) + 7 * bf16)
    for use in [(True, True), (True, False), (False, True), (False, False)]:
        if (mis == "ba" and not use[0]) or (mis == "bs" and not use[1]):
            continue
        assert run_add_bias_relu(L, bf16, n, C, inner, rng, use, mis, None, what=name) == want
    for alias in ("a", "s"):
        if (alias, mis) in (("a", 2), ("s", 2)):
            continue  # `out` is the aliased input: its offset is that input's
        run_add_bias_relu(L, bf16, n, C, inner, rng, (True, True), mis, alias, what=name)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", [c for c in CASE_NAMES if c not in ("vec_off_1", "vec_off_2", "vec_off_3",
                                                                     "vec_bias_s_off")])
def test_bias_act_routes(L, name, bf16):
    """wam_ew_bias_act (in place) on the rows of the route table that apply to one tensor and one
    bias: with and without the bias, relu = 0 and 1."""
    _, n, C, inner, mis, want, _ = _case(bf16, name)
    rng = np.random.RandomState(len(name) + 11 * bf16)
    for use in (True, False):
        if mis == "ba" and not use:
            continue
        for relu in (0, 1):
            assert run_bias_act(L, bf16, n, C, inner, rng, use, relu, mis, what=name) == want


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["vec", "ragged", "vec_off_0", "vec_off_1", "vec_off_2", "vec_off_3"])
def test_relu_mask_routes(L, name, bf16):
    """wam_ew_relu_mask: the 16-byte kernel, n % V != 0 and each of g1, g2, y, out one element off
    in turn; g2 NULL and not; out a buffer of its own, out == g1, out == g2 and out == y."""
    _, n, _, _, mis, want, _ = _case(bf16, name)
    want = "vec" if want == "CH_VEC" else want
    rng = np.random.RandomState(len(name) + 13 * bf16)
    for two in (True, False):
        if mis == 1 and not two:
            continue
        assert run_relu_mask(L, bf16, n, rng, two, mis, None, what=name) == want
        for alias in ("g1", "y") + (("g2",) if two else ()):
            if mis == 3:
                continue  # `out` is the aliased input
            run_relu_mask(L, bf16, n, rng, two, mis, alias, what=name)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nvec", [1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_vector_routes_at_workgroup_boundaries(L, nvec, bf16):
    """A workgroup of 256 threads moves 4 vectors per thread, thread t the vectors t, t + 256, t + 512,
    t + 768 of its 1,024: sizes on both sides of one unrolled step (256), of one workgroup (1,024)
    and of two (2,049), on CH_VEC (C = 3V, so the bias vector starts at c0 = 0, V or 2V), CH_ONE
    (inner = 2V, C = 5) and the 16-byte mask kernel."""
    V = V_of(bf16)
    n = nvec * V
    rng = np.random.RandomState(nvec + bf16)
    assert run_add_bias_relu(L, bf16, n, 3 * V, 1, rng, what="nvec %d" % nvec) == "CH_VEC"
    assert run_add_bias_relu(L, bf16, n, 5, 2 * V, rng, what="nvec %d" % nvec) == "CH_ONE"
    for relu in (0, 1):
        assert run_bias_act(L, bf16, n, 3 * V, 1, rng, True, relu, what="nvec %d" % nvec) == "CH_VEC"
        assert run_bias_act(L, bf16, n, 5, 2 * V, rng, True, relu, what="nvec %d" % nvec) == "CH_ONE"
    for two in (True, False):
        assert run_relu_mask(L, bf16, n, rng, two, what="nvec %d" % nvec) == "vec"


def _spliced(rng, n, bf16, p=None, q=None):
    """two operands of n ordinary values with every ordered pair of SPECIALS, then PAIRS, at the
    front (or: p / q given, one operand with SPECIALS cycling against it)"""
    k = len(SPECIALS)
    assert n >= k * k + len(PAIRS)
    a, s = values(rng, n, bf16), values(rng, n, bf16)
    a[:k * k], s[:k * k] = np.repeat(SPECIALS, k), np.tile(SPECIALS, k)
    for i, (u, v) in enumerate(PAIRS):
        a[k * k + i], s[k * k + i] = u, v
    return a, s


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["vec", "one", "ragged"])
def test_special_values(L, name, bf16):
    """NaN, +-inf, -0.0, the pair whose fp32 sum is the bf16 tie to infinity, FLT_MAX + FLT_MAX and the
    bf16 round-to-even ties in both directions, spliced into every operand -- every ordered pair of
    the special values in (a, s), (g1, g2), (g1, y), (y, bias) -- on CH_VEC, CH_ONE and the scalar
    kernel. The forward ReLU passes NaN on; the mask is 0 at a NaN, -0.0 or negative activation."""
    V = V_of(bf16)
    _, _, C, inner, _, want, _ = _case(bf16, name)
    n = {"vec": 216, "one": 240, "ragged": 219}[name]  # multiples of C * inner for both types (ragged: + 3)
    rng = np.random.RandomState(31 + bf16)
    k = len(SPECIALS)
    a, s = _spliced(rng, n, bf16)
    ref = R.add_bias_relu_ref(R.store(a, bf16), None, R.store(s, bf16), None, C, inner)
    assert np.isnan(ref[:k]).all() and np.isnan(ref).sum() > 2 * k - 2  # the reference itself propagates NaN
    for use in [(False, False), (True, True)]:
        assert run_add_bias_relu(L, bf16, n, C, inner, rng, use, a=a, s=s, what=name + " specials") == want
    # specials in the biases: channel c holds SPECIALS[(c + shift) % k], so 3 shifts of C >= 5 channels show them all
    for shift in (0, 5, 10):
        bsp = SPECIALS[(np.arange(C) + shift) % k]
        run_add_bias_relu(L, bf16, n, C, inner, rng, (True, True), a=a, s=s, ba=bsp, what=name + " special bias_a")
        run_add_bias_relu(L, bf16, n, C, inner, rng, (True, True), bs=bsp, what=name + " special bias_s")
        for relu in (0, 1):
            assert run_bias_act(L, bf16, n, C, inner, rng, True, relu, y=a, b=bsp, what=name + " special bias") == want
    # (y, bias) pairs of the tie list: the channel's elements get p, the channel's bias q
    ch = (np.arange(n) // inner) % C
    y, b = values(rng, n, bf16), values(rng, C, bf16)
    for c, (u, v) in enumerate(PAIRS[:C]):
        y[np.flatnonzero(ch == c)[:2]], b[c] = u, v
    for relu in (0, 1):
        run_bias_act(L, bf16, n, C, inner, rng, True, relu, y=y, b=b, what=name + " tie pairs")
        run_bias_act(L, bf16, n, C, inner, rng, False, relu, y=a, what=name + " specials, no bias")
    if name != "one":  # the mask has no channels: one vector route
        mw = "vec" if want == "CH_VEC" else want
        assert run_relu_mask(L, bf16, n, rng, True, g1=a, g2=s, what=name + " special g1, g2") == mw
        assert run_relu_mask(L, bf16, n, rng, True, g1=a, g2=s, y=np.abs(values(rng, n, bf16)) + 1,
                             what=name + " special g1, g2 under y > 0") == mw
        for two in (True, False):
            run_relu_mask(L, bf16, n, rng, two, g1=a, y=s, what=name + " special g1, y")
            run_relu_mask(L, bf16, n, rng, two, g1=np.ones(n, dtype=F32), y=s, what=name + " special y")


def test_elementwise_entry_validation(L):
    """n = 0 returns OK and writes nothing (NULL operands allowed); a bad dtype, channels < 1,
    inner < 1, n < 0 and NULL operands return WAM_ERR_INVALID_ARG and write nothing."""
    lib, st = L.lib, stream(L)
    rng = np.random.RandomState(0)
    for bf16 in (False, True):
        n, C = 64, 8
        dt = int(bf16)
        A, S, O = Buf(bf16, n, values(rng, n, bf16)), Buf(bf16, n, values(rng, n, bf16)), Buf(bf16, n)
        B = Buf(bf16, C, values(rng, C, bf16))
        calls = [
            (OK, lambda: lib.wam_ew_add_bias_relu(dt, 0, C, 1, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (OK, lambda: lib.wam_ew_add_bias_relu(dt, 0, C, 1, None, None, None, None, None, st)),
            (OK, lambda: lib.wam_ew_bias_act(dt, 0, C, 1, O.ptr, B.ptr, 1, st)),
            (OK, lambda: lib.wam_ew_relu_mask(dt, 0, A.ptr, S.ptr, A.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(2, n, C, 1, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(-1, n, C, 1, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, n, 0, 1, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, n, C, 0, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, -4, C, 1, A.ptr, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, n, C, 1, None, B.ptr, S.ptr, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, n, C, 1, A.ptr, B.ptr, None, B.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_add_bias_relu(dt, n, C, 1, A.ptr, B.ptr, S.ptr, B.ptr, None, st)),
            (INVALID, lambda: lib.wam_ew_bias_act(2, n, C, 1, O.ptr, B.ptr, 1, st)),
            (INVALID, lambda: lib.wam_ew_bias_act(dt, n, 0, 1, O.ptr, B.ptr, 1, st)),
            (INVALID, lambda: lib.wam_ew_bias_act(dt, n, C, 0, O.ptr, B.ptr, 1, st)),
            (INVALID, lambda: lib.wam_ew_bias_act(dt, n, C, 1, None, B.ptr, 1, st)),
            (INVALID, lambda: lib.wam_ew_relu_mask(2, n, A.ptr, S.ptr, A.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_relu_mask(dt, -1, A.ptr, S.ptr, A.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_relu_mask(dt, n, None, S.ptr, A.ptr, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_relu_mask(dt, n, A.ptr, S.ptr, None, O.ptr, st)),
            (INVALID, lambda: lib.wam_ew_relu_mask(dt, n, A.ptr, S.ptr, A.ptr, None, st)),
        ]
        for i, (want, fn) in enumerate(calls):
            assert fn() == want, "call %d" % i
        torch.cuda.synchronize()
        assert O.untouched()
        R.assert_same(A.read("validation"), A.vals, "validation input")


# ------------------------------------------------------------------------------ max pool
def _pool_fwd(L, bf16, x, k, s, p, what, off=(0, 0, 0)):
    n, h, w, c = x.shape
    ho, wo = R.pool_out(h, w, k, s, p)
    X = Buf(bf16, x.size, x.reshape(-1), off[0])
    Y = Buf(bf16, n * ho * wo * c, None, off[1])
    I = IdxBuf(n * ho * wo * c, None, off[2])
    rc = L.lib.wam_ew_maxpool_nhwc(int(bf16), n, h, w, c, k, s, p, X.ptr, Y.ptr, I.ptr, stream(L))
    torch.cuda.synchronize()
    return rc, X, Y, I


class IdxBuf:
    """the byte index of the pool inside 0xEE guards (no position | 0x80 is 0xEE: 0x6E = 110 needs
    k = 11, whose flagged last position is 248)"""
    FILL = 0xEE

    def __init__(self, n, vals=None, off=0):
        self.n, self.lo = n, PAD + off
        host = np.full(PAD + off + n + PAD, self.FILL, dtype=np.uint8)
        if vals is not None:
            host[self.lo:self.lo + n] = vals.reshape(-1)
        self.dev = torch.from_numpy(host).cuda()
        self.addr = self.dev.data_ptr() + self.lo

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def read(self, what):
        raw = self.dev.cpu().numpy()
        assert (raw[:self.lo] == self.FILL).all() and (raw[self.lo + self.n:] == self.FILL).all(), \
            "%s: a guard of the index was written" % what
        return raw[self.lo:self.lo + self.n]

    def untouched(self):
        return bool((self.dev.cpu().numpy() == self.FILL).all())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("k,s,p,h,w", R.GEOMS)
def test_maxpool_forward_and_backward(L, k, s, p, h, w, bf16):
    """wam_ew_maxpool_nhwc and wam_ew_maxpool_nhwc_backward, 2 images, c = V, 3V and 4V channels, the
    three input families of modelew_ref.pool_input: y and every index byte equal maxpool_ref (first
    maximum, last NaN, first valid position of a -inf window, bit 7 iff the maximum is > 0); the
    backward, fed the REFERENCE's index and a gradient whose float32 sums depend on their order,
    equals maxpool_bwd_ref on every element of a sentinel-filled gx -- the zeros of pixels no window
    covers included -- with relu = 0 and 1."""
    V = V_of(bf16)
    n = 2
    ho, wo = R.pool_out(h, w, k, s, p)
    for cm in (1, 3, 4):
        c = cm * V
        for family in ("ties", "negative", "special"):
            rng = np.random.RandomState(1000 * k + 100 * s + 10 * h + cm)
            what = "maxpool %s k%d s%d p%d %dx%d c=%d %s" % ("bf16" if bf16 else "fp32", k, s, p, h, w, c, family)
            x = R.pool_input(family, rng, n, h, w, c, k)
            rc, X, Y, I = _pool_fwd(L, bf16, x, k, s, p, what)
            assert rc == OK, what
            ry, ridx = R.maxpool_ref(x, k, s, p)
            got_idx = I.read(what).reshape(ridx.shape)
            bad = np.argwhere(got_idx != ridx)
            assert not len(bad), "%s: %d index bytes differ, first at %s: got %d, reference %d" % (
                what, len(bad), bad[0], got_idx[tuple(bad[0])], ridx[tuple(bad[0])])
            R.assert_same(Y.read(what).reshape(ry.shape), ry, what + " values")
            R.assert_same(X.read(what), X.vals, what + " input")
            if family == "negative":
                assert not (ridx & 0x80).any()
            gy = R.spread_grad(rng, ry.shape)
            for relu in (0, 1):
                GY = Buf(bf16, gy.size, gy.reshape(-1))
                II = IdxBuf(ridx.size, ridx)
                GX = Buf(bf16, x.size)
                rc = L.lib.wam_ew_maxpool_nhwc_backward(int(bf16), n, h, w, c, k, s, p, GY.ptr, II.ptr, relu, GX.ptr,
                                                        stream(L))
                torch.cuda.synchronize()
                assert rc == OK, what
                ref = R.maxpool_bwd_ref(GY.vals.reshape(ry.shape), ridx, x.shape, k, s, p, relu)
                check_out(GX, ref.reshape(-1), what + " backward relu=%d" % relu)
    if (k, s) == (2, 3):
        assert (np.arange(h) % s >= k).any()  # rows no window covers


def test_maxpool_largest_index_byte(L):
    """k = 11: a positive maximum at the window's last position gives 120 | 0x80 = 248, a negative
    one 120."""
    for bf16 in (False, True):
        V = V_of(bf16)
        x = np.full((1, 11, 11, V), -2.0, dtype=F32)
        x[0, 10, 10, ::2] = 3.0
        x[0, 10, 10, 1::2] = -1.0
        rc, _, Y, I = _pool_fwd(L, bf16, x, 11, 1, 0, "k=11")
        assert rc == OK
        assert np.array_equal(I.read("k=11"), np.tile(np.array([248, 120], dtype=np.uint8), V // 2))
        assert np.array_equal(Y.read("k=11"), np.tile(np.array([3.0, -1.0], dtype=F32), V // 2))


def test_maxpool_rejections(L):
    """WAM_ERR_UNSUPPORTED for c % V != 0, a misaligned x / y / gy / gx and a misaligned index;
    WAM_ERR_INVALID_ARG for k = 12, 2p > k, h = 0, an image smaller than the window and NULL pointers; n = 0 is
    OK. Every output still
    holds its sentinel."""
    lib, st = L.lib, stream(L)
    for bf16 in (False, True):
        V, dt = V_of(bf16), int(bf16)
        n, h, w, c, k, s, p = 2, 5, 4, 2 * V, 2, 2, 0
        ho, wo = R.pool_out(h, w, k, s, p)
        rng = np.random.RandomState(3)
        big = n * h * w * (c + 1)
        outs = []

        def fwd(c_=c, k_=k, p_=p, h_=h, w_=w, n_=n, ox=0, oy=0, oi=0, null=None):
            X, Y, I = Buf(bf16, big, values(rng, big, bf16), ox), Buf(bf16, big, None, oy), IdxBuf(big, None, oi)
            outs.extend([Y, I])
            a = [None if null == i else b.ptr for i, b in enumerate((X, Y, I))]
            return lib.wam_ew_maxpool_nhwc(dt, n_, h_, w_, c_, k_, s, p_, a[0], a[1], a[2], st)

        def bwd(c_=c, k_=k, p_=p, h_=h, w_=w, n_=n, og=0, oi=0, ox=0, null=None):
            GY = Buf(bf16, big, values(rng, big, bf16), og)
            I = IdxBuf(big, np.zeros(big, dtype=np.uint8), oi)
            GX = Buf(bf16, big, None, ox)
            outs.append(GX)
            a = [None if null == i else b.ptr for i, b in enumerate((GY, I, GX))]
            return lib.wam_ew_maxpool_nhwc_backward(dt, n_, h_, w_, c_, k_, s, p_, a[0], a[1], 1, a[2], st)

        assert fwd(c_=c + 1) == UNSUPPORTED and bwd(c_=c + 1) == UNSUPPORTED
        assert fwd(c_=V // 2) == UNSUPPORTED and bwd(c_=V // 2) == UNSUPPORTED
        assert fwd(ox=1) == UNSUPPORTED and fwd(oy=1) == UNSUPPORTED
        assert bwd(og=1) == UNSUPPORTED and bwd(ox=1) == UNSUPPORTED
        for oi in (1, V // 2):  # the index is moved V bytes at a time
            assert fwd(oi=oi) == UNSUPPORTED and bwd(oi=oi) == UNSUPPORTED
        assert fwd(k_=12, p_=0) == INVALID and bwd(k_=12, p_=0) == INVALID
        assert fwd(k_=3, p_=2) == INVALID and bwd(k_=3, p_=2) == INVALID
        assert fwd(h_=0) == INVALID and bwd(h_=0) == INVALID
        assert fwd(k_=0) == INVALID and bwd(k_=0) == INVALID
        # an image smaller than the window, padding included, has no output (torch raises)
        assert fwd(h_=1) == INVALID and bwd(h_=1) == INVALID and fwd(w_=1) == INVALID and bwd(w_=1) == INVALID
        for i in range(3):
            assert fwd(null=i) == INVALID and bwd(null=i) == INVALID
        assert lib.wam_ew_maxpool_nhwc(2, n, h, w, c, k, s, p, outs[0].ptr, outs[0].ptr, outs[1].ptr, st) == INVALID
        assert fwd(n_=0) == OK and bwd(n_=0) == OK
        assert fwd(n_=0, null=1) == OK
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)


# ------------------------------------------------------------------------------ wrappers
def _exact(gen, shape, dtype):
    """multiples of 1/16 in [-4, 4]: exact in bf16, and every sum of four of them is exact in fp32,
    so the float64 expression cast to the dtype is the kernel's result bit for bit"""
    return (torch.randint(-64, 65, shape, generator=gen, device="cuda").float() / 16).to(dtype)


def _bc(b, t):
    return b.double().reshape((1, -1) + (1,) * (t.dim() - 2))


WRAP_SHAPES = [(3, 10), (2, 6, 9), (2, 5, 2, 3, 4), (3, 1, 5, 6), (4, 12, 1, 1), (2, 8, 5, 6)]


def _variants(t):
    """the same values as: dense, every second element of a wider tensor, a slice of a longer batch,
    and (4-D) channels_last -- a fresh tensor each (bias_act_ works in place where it can)"""
    yield "dense", t.clone()
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    yield "strided", wide[..., ::2]
    longer = lambda: torch.cat([torch.full_like(t[:1], 7.0), t, torch.full_like(t[:1], -7.0)])  # noqa: E731
    yield "sliced", longer()[1:-1]
    if t.dim() == 4:
        yield "channels_last", t.clone().contiguous(memory_format=torch.channels_last)
        yield "channels_last sliced", longer().contiguous(memory_format=torch.channels_last)[1:-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", WRAP_SHAPES)
def test_wrappers_take_any_layout(L, shape, dtype):
    """model_fuse.bias_act_ / add_bias_relu / relu_mask vs the same expression in torch float64 cast to
    the dtype (equal: see _exact), for [N, C], [N, C, L], [N, C, D, H, W], [N, 1, H, W], [N, C, 1, 1]
    and [N, C, H, W] operands that are dense, strided, sliced or channels_last in every combination
    of (first, second) operand, and a bias expanded from one element."""
    from wam_amd import model_fuse as mf
    gen = torch.Generator(device="cuda").manual_seed(sum(shape))
    C = shape[1]
    a, s, g, g2 = (_exact(gen, shape, dtype) for _ in range(4))
    y = torch.relu(_exact(gen, shape, dtype))
    y[y == 0.5] = -0.0
    b1, b2 = _exact(gen, (C,), dtype), _exact(gen, (C,), dtype)
    one = torch.full((1,), 0.75, device="cuda", dtype=dtype).expand(C)
    z = torch.zeros(shape, dtype=torch.float64, device="cuda")
    for b in (b1, one, None):
        pre = a.double() + (_bc(b, a) if b is not None else 0)
        for relu in (True, False):
            ref = (torch.relu(pre) if relu else pre).to(dtype)
            for name, av in _variants(a):
                assert torch.equal(mf.bias_act_(av, b, relu), ref), (name, relu)
    ref = torch.relu((a.double() + _bc(b1, a)) + (s.double() + _bc(one, s))).to(dtype)
    ref0 = torch.relu(a.double() + s.double()).to(dtype)
    rm = torch.where(y > 0, g.double(), z).to(dtype)
    rm2 = torch.where(y > 0, g.double() + g2.double(), z).to(dtype)
    for na, av in _variants(a):
        for ns, sv in _variants(s):
            assert torch.equal(mf.add_bias_relu(av, b1, sv, one), ref), (na, ns)
            assert torch.equal(mf.add_bias_relu(av, None, sv, None), ref0), (na, ns)
    for ny, yv in _variants(y):
        for ng, gv in _variants(g):
            assert torch.equal(mf.relu_mask(gv, yv), rm), "relu_mask: y %s, g %s" % (ny, ng)
            assert torch.equal(mf.relu_mask(gv, yv, g2), rm2), "relu_mask with g2: y %s, g %s" % (ny, ng)
            # g2 in every layout too (the same values as g: the sum is 2 g)
            assert torch.equal(mf.relu_mask(g, yv, gv), torch.where(y > 0, 2 * g.double(), z).to(dtype)), (ny, ng)
