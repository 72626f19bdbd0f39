"""CPU tier: the f16 screen of the pruned sum-only d = 8 sweep (csrc/kde_screen_d8.inc) - its error bound restated in numpy, and its listing.

The screen drops a (tile, group) block only when every pair's approximate exponent plus its error bound lies below the group's threshold.  The
bound is E = e_t + e_q with e = KAPPA N + LAMBDA R + MU per row (N = 1/2|z|^2, R = |z|), derived in the source and in DESIGN.md 3.1; here the
operands are built as kde_screen_pack_kernel builds them (np.float16, nothing subnormal, hi + lo norms, shares of the bound rounded up), the 16
products are accumulated in float32 in the matrix core's k order, and |s~ - s| <= E is held against the fp64 exponent on rows chosen to hurt.
An order-independent form is held too: the exactly summed f16 operands plus 17 x 2^-23 of the products' magnitudes."""
import re

import numpy as np
import pytest

from helpers import unit_asm

KAPPA = 2.0 ** -10 + 2.0 ** -20 + 35.0 * 2.0 ** -23
LAMBDA = 2.0 ** -12
MU = 2.0 ** -13


def h_piece(x):
    """f16 by way of fp32, never subnormal (kde_kernels.hpp: h_piece)."""
    h = np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float16)
    return np.where(np.abs(h.astype(np.float64)) < 2.0 ** -14, np.float16(0), h)


def f16_up(x):
    h = np.asarray(x, dtype=np.float64).astype(np.float16)
    low = h.astype(np.float64) < x
    return np.where(low, (h.view(np.uint16) + np.uint16(1)).view(np.float16), h)


def pack(z, query):
    """[n][16] float16 operands of rows z [n][8] and the rows' flags."""
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = np.zeros(n)
        for k in range(8):
            n2 = z[:, k] * z[:, k] + n2
        N = 0.5 * n2
        ok = np.all(np.abs(z) <= 65504.0, axis=1) & (N <= 60000.0)
    zz = np.where(ok[:, None], z, 0.0)
    Nn = np.where(ok, N, 0.0)
    out = np.zeros((n, 16), dtype=np.float16)
    out[:, :8] = h_piece(zz)
    hi = h_piece(-Nn)
    lo = h_piece(-Nn - hi.astype(np.float64))
    e = f16_up(KAPPA * Nn + LAMBDA * np.sqrt(2.0 * Nn) + MU)
    hi = np.where(ok, hi, np.float16(np.inf))
    lo = np.where(ok, lo, np.float16(0))
    e = np.where(ok, e, np.float16(0))
    one = np.float16(1)
    if query:
        out[:, 8:11] = one
        out[:, 12], out[:, 13], out[:, 14] = hi, lo, e
    else:
        out[:, 8], out[:, 9], out[:, 10] = hi, lo, e
        out[:, 12:15] = one
    return out, ok


def mfma_f32(a, b, slots):
    """sum over `slots` of a[t, k] b[q, k] as a k-ordered float32 chain from 0: [nt][nq] float32."""
    acc = np.zeros((len(a), len(b)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in slots:
            p = (a[:, k].astype(np.float64)[:, None] * b[:, k].astype(np.float64)[None, :]).astype(np.float32)   # exact: 11 x 11 bits
            acc = (acc + p).astype(np.float32)
    return acc


def adversarial(rng, n):
    """Whitened rows [n][8]: a correlated cloud at the bench table's scale, then rows chosen to hurt."""
    mix = np.tril(np.full((8, 8), 0.3), -1) + np.eye(8)
    z = rng.normal(size=(n, 8)) @ mix.T * 3.8
    z[0] = 40.0
    z[1] = -40.0
    z[2] = 60.0
    z[3] = -60.0
    z[4] = [40.0, -40.0, 60.0, -60.0, 0.0, 1e-9, -1e-9, 86.0]
    # f16 rounding midpoints: halfway between neighbours at several magnitudes
    z[5] = [1.0 + 2.0 ** -11, 2.0 + 2.0 ** -10, 32.0 + 2.0 ** -6, -(64.0 + 2.0 ** -5), 0.5 + 2.0 ** -12, 3.0 * 2.0 ** -11, -(1.0 - 2.0 ** -12), 16.0 + 2.0 ** -7]
    z[6] = -z[5]
    # f16 subnormals and their neighbourhood
    z[7] = [2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -15, -(2.0 ** -14), 2.0 ** -14 * (1 - 2.0 ** -12), 3e-6, -5.9e-8, 6.1e-5]
    z[8] = z[7] * 40.0 * 2.0 ** 14
    z[9:19] = z[20]        # duplicated rows
    z[19] = 0.0
    z[21] = 108.0          # N = 46 656: inside the operands' range, near its end
    z[22] = -122.0         # N = 59 536
    return z


def test_bound_holds_on_adversarial_rows():
    rng = np.random.default_rng(11)
    zt = adversarial(rng, 700)
    zq = adversarial(rng, 300)
    zq[30:130] = zt[:100]               # queries on training rows
    zq[130:160] = zt[:30] + 2.0 ** -12  # and a hair off them
    a, okt = pack(zt, False)
    b, okq = pack(zq, True)
    assert okt.all() and okq.all()
    s = zt @ zq.T - 0.5 * np.sum(zt * zt, axis=1)[:, None] - 0.5 * np.sum(zq * zq, axis=1)[None, :]
    approx = mfma_f32(a, b, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]).astype(np.float64)
    E = a[:, 10].astype(np.float64)[:, None] + b[:, 14].astype(np.float64)[None, :]
    err = np.abs(approx - s)
    print(f"max |s~ - s| / E = {np.max(err / E):.3f}; median E = {np.median(E):.4f}, largest E = {E.max():.3f}")
    assert np.all(err <= E)
    # what the kernel compares: the chain with the bound's slots in it is never below the exact exponent
    full = mfma_f32(a, b, range(16)).astype(np.float64)
    assert np.all(full >= s)
    # order-independent: the exact sum of the f16 operands, and any fp32 summation of 16 products (17 x 2^-23 of their magnitudes)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    use = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]
    exact = a64[:, use] @ b64[:, use].T
    T = np.abs(a64) @ np.abs(b64).T
    assert np.all(np.abs(exact - s) + 17.0 * 2.0 ** -23 * T <= E)


def test_bound_holds_on_random_tables():
    rng = np.random.default_rng(12)
    for scale in (0.01, 1.0, 3.8, 25.0):
        mix = np.tril(np.full((8, 8), 0.3), -1) + np.eye(8)
        zt = rng.normal(size=(1500, 8)) @ mix.T * scale
        zq = rng.standard_t(3, size=(500, 8)) * scale
        a, okt = pack(zt, False)
        b, okq = pack(zq, True)
        s = zt @ zq.T - 0.5 * np.sum(zt * zt, axis=1)[:, None] - 0.5 * np.sum(zq * zq, axis=1)[None, :]
        approx = mfma_f32(a, b, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]).astype(np.float64)
        E = a[:, 10].astype(np.float64)[:, None] + b[:, 14].astype(np.float64)[None, :]
        live = okt[:, None] & okq[None, :]
        assert np.all((np.abs(approx - s) <= E)[live])


def test_rows_beyond_the_operands_are_kept():
    rng = np.random.default_rng(13)
    zt = adversarial(rng, 64)
    zq = adversarial(rng, 64)
    bad = [[np.nan] + [0.0] * 7, [np.inf] * 8, [-np.inf, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [70000.0] + [0.0] * 7, [200.0] * 8, [-1e300] * 8]
    zt[40:46] = bad
    zq[50:56] = bad
    a, okt = pack(zt, False)
    b, okq = pack(zq, True)
    assert not okt[40:46].any() and not okq[50:56].any() and okt[:40].all() and okq[:50].all()
    full = mfma_f32(a, b, range(16))
    flagged = ~okt[:, None] | ~okq[None, :]
    assert np.all(full[flagged] == np.inf)          # never a NaN, which a maximum would lose
    assert np.all(np.isfinite(full[~flagged]))
    for thr in (np.float32(-50.0), np.float32(3e38), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)):
        with np.errstate(invalid="ignore"):
            dead = full < thr                            # the kernel keeps on !(max < thr)
        assert not dead[flagged].any(), thr
    with np.errstate(invalid="ignore"):
        assert not (full < np.float32(np.nan)).any()     # a NaN threshold keeps everything


@pytest.fixture(scope="module")
def kde_asm():
    return unit_asm("kde_kernels")


def kernel(asm, name):
    hdr = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, flags=re.S).group(1)
    body = next(f for f in re.split(r"\n(?=_Z[A-Za-z0-9_]+:)", asm) if f.startswith(name + ":")).split(".Lfunc_end")[0]
    return hdr, body


def test_screen_kernel_listing(kde_asm):
    hdr, body = kernel(kde_asm, "_ZN3pbn20kde_screen_d8_kernelENS_9SweepArgsE")
    assert "v_mfma_f32_32x32x16_f16" in body
    assert "v_mfma_f64" not in body
    assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0 and "scratch_" not in body
    assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 128   # four waves per SIMD: the walk is latency


def test_sweep_reads_prepared_masks_into_scalar_registers(kde_asm):
    """With SweepArgs::live_mask the d = 8 sweep loads a super-batch's mask words lane = batch and hands a batch its own with v_readlane_b32 (two
    groups x two halves): the words are then tested in scalar registers like the masks of its own box tests (the bodies hold no v_cmp_ne_u64:
    tests/test_isa_prune_d8_cpu.py)."""
    hdr, body = kernel(kde_asm, "_ZN3pbn26kde_sweep_pruned_d8_kernelENS_9SweepArgsE")
    assert len(re.findall(r"\bv_readlane_b32 s", body)) >= 4
    assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 168
    assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0 and "scratch_" not in body
