"""tools/prune_window_estimate.py (the window-sum bound's estimator): the bound lies below every query's exact log2 sum, tightens with the
window, and prunes at least as much as the prepass bound on a small table."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import prune_d8_estimate as E  # noqa: E402
import prune_window_estimate as W  # noqa: E402


def test_window_bound_is_a_lower_bound_that_tightens():
    tr, te = E.bench_table(16 * 2000 + 7, 0), E.bench_table(16 * 40, 1)
    h = E.normal_reference_diag(tr)
    ztr, zte = tr * np.sqrt(E.LOG2E / h), te * np.sqrt(E.LOG2E / h)
    R, _ = E.principal_rotation(ztr)
    zt, zq = ztr @ R.T, zte @ R.T
    tk, qk = E.morton_keys(zt), E.morton_keys(zq)
    tperm, qperm = np.argsort(tk, kind="stable"), np.argsort(qk, kind="stable")
    zts, zqs = zt[tperm], zq[qperm]
    tpos = np.searchsorted(tk[tperm], qk[qperm]).reshape(-1, 16)
    zg = zqs.reshape(-1, 16, E.D)
    exact = E.log2_sums(zqs, zts).reshape(-1, 16).min(1)
    prev = np.full(zg.shape[0], -np.inf)
    for w in (4, 64, 4096):
        wb = np.array([W.window_bound(zg[i], int(tpos[i][0]) // 16, zts, w) for i in range(zg.shape[0])])
        assert np.all(wb <= exact + 1e-9)
        assert np.all(wb >= prev - 1e-9)
        prev = wb
    # a window over the whole table: the exact bound less the slack
    assert np.allclose(prev, exact - W.SLACK, atol=1e-9)
    lo_t, hi_t = E.tile_boxes(zts, E.D)
    glo, ghi = zg.min(1), zg.max(1)
    pre = np.array([E.prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t) for i in range(zg.shape[0])])
    v_pre, _ = W.block_fractions(lo_t, hi_t, glo, ghi, pre)
    v_win, far = W.block_fractions(lo_t, hi_t, glo, ghi, np.maximum(pre, prev))
    v_ex, _ = W.block_fractions(lo_t, hi_t, glo, ghi, exact)
    assert v_ex <= v_win + 1e-12 and v_win <= v_pre + 1e-12 and 0.0 <= far <= 1.0
