"""GPU: per-impression ROC-AUC and top-1 hit (pool_loss.hip: row_auc_kernel through the C ABI nrm_row_auc) against the oracle's row_auc
and numpy.argmax on the cases of row_auc_util: lanes that take several candidates, ties everywhere, lengths of 0, 1, T, beyond T and
below 0, padding that would win, labels of exactly 0.5, and equal maxima in different lanes and in one lane.

gt, eq and the class counts are integers below 2^24 (test_row_auc_cpu.py asserts n_pos n_neg < 2^24 for the cases), exact in fp32;
auc = (gt + 0.5 eq) / (n_pos n_neg) then takes an addition, a product and a division: |auc - auc64| <= 3 * 2^-24 auc64.  top1 is exact.

Measured on MI355X (20 cases, 0.1 s): worst |auc - auc64| / bound 0.30.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import row_auc_util as ru  # noqa: E402
from news_recommendation_model_amd import native  # noqa: E402

WORST = [0.0]


def _row_auc(lib, case):
    B, T = case.score.shape
    s, y = torch.from_numpy(case.score).cuda(), torch.from_numpy(case.label).cuda()
    ln = torch.from_numpy(case.length).cuda() if case.length is not None else None
    auc = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda")        # one entry more than the call writes
    top1 = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    rc = lib.nrm_row_auc(native.ptr(s), native.ptr(y), native.ptr(ln) if ln is not None else None, B, T, native.ptr(auc), native.ptr(top1),
                         native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.nrm_last_error()
    auc, top1 = auc.cpu().numpy(), top1.cpu().numpy()
    assert np.isnan(auc[B]) and top1[B] == -7, case.name
    return auc[:B], top1[:B]


@pytest.mark.parametrize("case", ru.all_cases(), ids=lambda c: c.name)
def test_auc_and_top1(lib, case):
    auc, top1 = _row_auc(lib, case)
    want_auc, want_top1, pairs = ru.reference(case)
    assert np.array_equal(top1, want_top1), case.name
    none = pairs == 0
    assert np.all(auc[none] == -1.0), case.name
    err, bound = np.abs(auc[~none].astype(np.float64) - want_auc[~none]), 3 * ru.U * want_auc[~none]
    assert np.all(err <= bound), (case.name, err, bound)
    if (bound > 0).any():
        WORST[0] = max(WORST[0], float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"{case.name}: worst |auc - auc64| / bound so far {WORST[0]:.3f}")


def test_zz_worst_ratio():
    print("worst |auc - auc64| / bound:", round(WORST[0], 3))
    assert WORST[0] <= 1.0
