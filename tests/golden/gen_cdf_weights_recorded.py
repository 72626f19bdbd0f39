"""Writes tests/golden/cdf_weights_recorded.npz: CKDE.cdf, CKDE.sample and UCV.score results of the library as built, on the inputs of
test_unwidened_results_unchanged (tests/test_cdf_weights_shapes_gpu.py) and test_ucv_f64_results_unchanged (tests/test_ucv_shapes_gpu.py).

The committed file was written with the library built from commit 8bfb9b6 - the last one whose fp32 cdf / sample / UCV fragments were
always floats - on an MI355X:  git checkout 8bfb9b6 -- pybnesian_amd/csrc && make -C pybnesian_amd/csrc && python tests/golden/gen_cdf_weights_recorded.py
Regenerating it from a later library only re-records that library's results: do so after a toolchain change moved the last bits, and
only once the two tests were seen to fail for that reason alone."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pybnesian_amd as pbn  # noqa: E402
import test_cdf_weights_shapes_gpu as T  # noqa: E402
import test_ucv_shapes_gpu as U  # noqa: E402

pbn.load_library()
out = {}
for p in (3, 9):
    data = T.random_table(90 + p, 1237 + 77, p)
    H = T.normal_reference(data, 1237)
    for dtype in T.DTYPES:
        d = T.rounded(data, dtype)
        out[f"cdf_{dtype}_{p}"] = T.fitted(pbn, d[:1237], H, dtype).cdf(T.frame(d[1237:], dtype))
for p in (2, 5):
    data = T.random_table(30 + p, 1500 + 700, p)
    H = T.normal_reference(data, 1500)
    for dtype in T.DTYPES:
        d = T.rounded(data, dtype)
        cpd = T.fitted(pbn, d[:1500], H, dtype)
        out[f"sample_{dtype}_{p}"] = cpd.sample(700, T.frame(d[1500:], dtype).iloc[:, 1:], 9).to_numpy().astype(np.float64)
ucv = pbn.UCV()
for n, d in ((257, 1), (700, 2), (611, 16), (903, 17)):
    x = U.table(n, d, 3 + d)
    H = U.normal_reference(np.cov(x.T).reshape(d, d), n)
    out[f"ucv_{n}_{d}"] = np.array([ucv.score(U.frame(x), U.cols(d), H), ucv.score(U.frame(x), U.cols(d), 0.3 * np.diag(H))])
np.savez(os.path.join(HERE, "cdf_weights_recorded.npz"), **out)
