"""CPU tier: the far pass's error bound, its theta rule and its kernel's listing (csrc/kde_far32_d8.inc).

The bound of |x32 - x| is restated here from the kernel's header and held against a numpy emulation of the fp32 evaluation - operands, norm
and constant rounded to fp32, eight products into the constant in fp32, fused and unfused, in several orders - on rows built against it:
every coordinate at the cap, coordinates on the midpoints of fp32 roundings, q = +-t, the offset at both ends of its range.  The emulation
must also REACH a stated fraction of the bound: the operand line of the bound, which the midpoint rows attain, is 1/45 of the whole at the
shipped cap (the rest prices the matrix core's ten operations at twice a rounding to nearest each, all of one sign, on the addends' full
magnitude); the test asks for 1/50.  The theta rule: the smallest integer with 10^6 2^-theta eps <= 8e-8, moving with log2(N / 10^6); the
library's own numbers (pbn_debug_far32_rule) are held to the restatement.  The listing: per (tile, group) block two v_mfma_f32_16x16x4_f32 and
four v_exp_f32, no fp64 MFMA, no packed fp32, no scratch, within the registers of four waves per SIMD."""
import ctypes
import itertools
import math
import re

import numpy as np
import pytest

from helpers import CSRC, unit_asm
from test_isa_screen_cpu import kernel

U, V = 2.0 ** -24, 2.0 ** -23
BUDGET = 8e-8
FAR = "_ZN3pbn25kde_sweep_far32_d8_kernelENS_9SweepArgsE"


def header_constant(name):
    with open(f"{CSRC}/kde_kernels.hpp") as f:
        return float(re.search(rf"^#define {name} ([0-9.e+-]+)", f.read(), flags=re.M).group(1))


NCAP, BIAS = header_constant("PBN_FAR32_NCAP"), header_constant("PBN_FAR32_BIAS")


def delta(C, B=None):
    """The header's bound of |x32 - x|, exponent units."""
    B = BIAS if B is None else B
    K = 5.0 * C + B + 1.0
    return (2 * U + U * U) * 2 * C + U * C + U * K + U * (1 + U) * (C + K) + ((1 + V) ** 10 - 1) * (1 + U) ** 2 * (3 * C + K)


def eps(C):
    return 2.0 ** delta(C) * (1 + V) * (1 + U) ** 255 - 1.0


def theta_1e6(C):
    return math.ceil(math.log2(1e6 * eps(C) / BUDGET))


def emulate(zt, zq, off, order, fused):
    """x32 of the kernel for rows zt, zq [n][8] (fp64) and integer offsets off [n]: fp32 all the way."""
    f = np.float32
    a, b = zt.astype(f), zq.astype(f)
    nt = (-0.5 * np.sum(zt * zt, axis=1)).astype(f)
    cq = (-0.5 * np.sum(zq * zq, axis=1) - off + BIAS).astype(f)
    acc = (cq + nt).astype(f)
    for k in order:
        if fused:   # one rounding per product-and-add (the product of two fp32 is exact in fp64)
            acc = (acc.astype(np.float64) + a[:, k].astype(np.float64) * b[:, k].astype(np.float64)).astype(f)
        else:
            acc = (acc + (a[:, k] * b[:, k]).astype(f)).astype(f)
    return acc.astype(np.float64)


def exact(zt, zq, off):
    """x in extended precision (the cancellation of three sums of a few hundred units each is below 1e-13 in longdouble)."""
    L = np.longdouble
    t, q = zt.astype(L), zq.astype(L)
    return np.asarray(np.sum(t * q, axis=1) - np.sum(t * t, axis=1) / 2 - np.sum(q * q, axis=1) / 2 - off.astype(L) + L(BIAS), dtype=np.float64)


def midpoint(x):
    """The fp64 number halfway between fp32(x) and its upper neighbour: the largest rounding error an operand can carry."""
    lo = x.astype(np.float32)
    hi = np.nextafter(lo, np.float32(np.inf))
    return (lo.astype(np.float64) + hi.astype(np.float64)) / 2


def attack_rows(C, rng):
    """Rows with 1/2|z|^2 <= C built against the bound; offsets over their whole range |off| <= 4 C + 1."""
    r = math.sqrt(2 * C / 8)
    rows = []
    base = np.full((1, 8), r * (1 - 1e-6))                                  # every coordinate at the cap
    rows += [base, -base]
    for _ in range(64):                                                     # ... with signs, on midpoints of fp32 roundings
        s = rng.choice([-1.0, 1.0], size=(1, 8))
        z = midpoint(np.abs(base) * rng.uniform(0.9, 1.0, size=(1, 8)) * (1 - 1e-6))
        rows.append(s * z)
    for _ in range(64):                                                     # one large coordinate, the others small
        z = rng.uniform(-1, 1, size=(1, 8)) * 0.1
        z[0, rng.integers(8)] = math.sqrt(2 * C) * 0.99
        rows.append(midpoint(np.abs(z)) * np.sign(z))
    z = np.vstack(rows)
    n = 0.5 * np.sum(z * z, axis=1)
    z *= np.minimum(1.0, np.sqrt(C / n * (1 - 1e-9)))[:, None]
    assert np.all(0.5 * np.sum(z * z, axis=1) <= C)
    zt, zq, off = [], [], []
    for t in z:
        for q in (t, -t, z[rng.integers(len(z))]):                          # q = +-t and a random partner
            for o in (-(4 * C + 1), -round(2 * C), 0, 4 * C + 1):
                zt.append(t), zq.append(q), off.append(float(o))
    return np.array(zt), np.array(zq), np.array(off)


def test_emulation_meets_the_bound_and_is_not_far_inside_it():
    rng = np.random.default_rng(16)
    for C in (NCAP, 64.0, 1000.0):
        zt, zq, off = attack_rows(C, rng)
        x = exact(zt, zq, off)
        worst = 0.0
        orders = [tuple(range(8)), tuple(reversed(range(8)))] + [tuple(rng.permutation(8)) for _ in range(6)]
        for order, fused in itertools.product(orders, (True, False)):
            worst = max(worst, float(np.max(np.abs(emulate(zt, zq, off, order, fused) - x))))
        print(f"NCAP {C:g}: worst |x32 - x| {worst:.3e} units over {len(x)} pairs x {2 * len(orders)} forms; bound {delta(C):.3e} ({worst / delta(C):.3f} of it)")
        assert worst <= delta(C), (C, worst, delta(C))
        assert worst >= delta(C) / 50.0, (C, worst, delta(C))


def test_theta_rule():
    th = theta_1e6(NCAP)
    print(f"NCAP {NCAP:g}, bias {BIAS:g}: delta {delta(NCAP):.3e} units, eps {eps(NCAP):.3e}, theta at 1e6 rows {th}")
    assert 1e6 * 2.0 ** -th * eps(NCAP) <= BUDGET < 1e6 * 2.0 ** -(th - 1) * eps(NCAP)
    assert th == 35   # the shipped constants


def test_the_library_follows_the_rule(ensure_built):
    import pybnesian_amd._lib as L

    lib = ctypes.CDLL(L.LIB_PATH)
    lib.pbn_debug_far32_rule.argtypes = [ctypes.c_double, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.pbn_debug_far32_rule.restype = None
    e, t = ctypes.c_double(), ctypes.c_double()
    for n in (1_000_000, 2_000_000, 131_087, 32_768, 4_000_000):
        lib.pbn_debug_far32_rule(NCAP, n, ctypes.byref(e), ctypes.byref(t))
        assert abs(e.value - eps(NCAP)) <= 1e-12 * eps(NCAP), (e.value, eps(NCAP))
        assert abs(t.value - (theta_1e6(NCAP) + math.log2(n / 1e6))) <= 1e-12, (n, t.value)
        assert n * 2.0 ** -t.value * e.value <= BUDGET * (1 + 1e-12)       # the same 8e-8 at every size
    lib.pbn_debug_far32_rule(1000.0, 1_000_000, ctypes.byref(e), None)
    assert abs(e.value - eps(1000.0)) <= 1e-12 * eps(1000.0)


@pytest.fixture(scope="module")
def kde_asm():
    return unit_asm("kde_kernels")


def test_far_kernel_listing(kde_asm):
    hdr, body = kernel(kde_asm, FAR)
    ins = [line.strip() for line in body.splitlines() if line.strip() and not line.strip().startswith((";", "."))]
    mfma = sum(i.startswith("v_mfma_f32_16x16x4_f32") for i in ins)
    ex = sum(i.startswith("v_exp_f32") for i in ins)
    vgpr = int(re.search(r"next_free_vgpr (\d+)", hdr).group(1))
    print(f"far kernel: {mfma} fp32 MFMAs, {ex} v_exp_f32, {vgpr} VGPRs")
    # the block body exists once per slot of the ring and group (two)
    with open(f"{CSRC}/kde_far32_d8.inc") as f:
        blocks = 2 * int(re.search(r"^#define PBN_FAR32_RING (\d+)", f.read(), flags=re.M).group(1))
    assert mfma == 2 * blocks and ex == 4 * blocks, (mfma, ex, blocks)
    assert not [i for i in ins if i.startswith("v_mfma") and "f64" in i], "no fp64 MFMA"
    assert not [i for i in ins if i.startswith("v_pk_")], "no packed fp32 beside the MFMAs"
    assert vgpr <= 128
    assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0 and "scratch_" not in body
