"""CPU: the float64 statements of pool_util against float64 torch.bmm; the float32 fused-multiply-add chain emulation of both pool kernels
-- in j order and in the four quarters of the JSPLIT form -- inside the bound on every case the GPU test runs; and every mutant
rejected at >= 4 x the bound on every case it applies to, by the same ``check_bmm`` / ``check_rowdot`` the GPU test applies."""
import numpy as np
import pytest
import torch

import pool_util as pu


def _bmm_cases(shapes=None):
    for B, I, J, D in (shapes or pu.bmm_shapes()):
        for layout in pu.LAYOUTS:
            for ldx in (D, D + 4):
                for family in pu.BMM_FAMILIES:
                    yield pu.make_bmm(B, I, J, D, layout, ldx, family)


def test_statements_match_float64_bmm():
    for c in _bmm_cases([(3, 17, 33, 68), (1, 1, 1, 4), (3, 65, 130, 68)]):
        B, I, J, D = c["B"], c["I"], c["J"], c["D"]
        wsb, wsi, wsj = c["strides"]
        W = torch.from_numpy(c["wmem"][:B * I * J]).double().as_strided((B, I, J), (wsb, wsi, wsj))
        X = torch.from_numpy(c["xmem"][:B * J * c["ldx"]]).double().reshape(B, J, c["ldx"])[:, :, :D]
        want = torch.bmm(W, X).numpy()
        assert np.abs(c["ref"] - want).max() <= 1e-13 * np.abs(want).max()
        ref, bound = pu.bmm_bound(c, 1)
        assert np.abs(ref - (want + c["prior"].astype(np.float64))).max() <= 1e-13 * np.abs(ref).max() and np.all(bound > 0)
    for B, T, H, D in ((3, 17, 65, 36), (1, 1, 1, 4)):
        for ldg in (D, D + 4):
            c = pu.make_rowdot(B, T, H, D, ldg, "normal")
            g = torch.from_numpy(c["gmem"][:B * T * ldg]).double().reshape(B, T, ldg)[:, :, :D]
            h = torch.from_numpy(c["hmem"][:B * H * D]).double().reshape(B, H, D)
            assert np.abs(c["ref"] - torch.bmm(g, h.transpose(1, 2)).numpy()).max() <= 1e-13 * np.abs(c["ref"]).max()


def test_the_dispatch_rule_of_the_emulation():
    """bmm_rows_plan: JSPLIT where there are at most 1024 tasks and J >= 32 -- both forms occur among the cases as dispatched"""
    taken = {pu.jsplit_taken(None, *s) for s in pu.bmm_shapes()}
    assert taken == {False, True}
    assert pu.jsplit_taken(None, 3, 17, 32, 68) and not pu.jsplit_taken(None, 3, 17, 31, 68) and not pu.jsplit_taken(None, 1025, 1, 32, 4)
    assert pu.jsplit_taken("1", 3, 1, 1, 4) and not pu.jsplit_taken("0", 3, 17, 130, 68)


@pytest.mark.parametrize("form", ["0", "1"])
def test_bmm_emulation_stays_inside_the_bound(form):
    be, worst = pu.Emulated(), 0.0
    for c in _bmm_cases():
        for accumulate in (0, 1):
            res = pu.check_bmm(be, c, accumulate, form)
            assert all(v <= 1.0 for v in res.values()), (c["B"], c["I"], c["J"], c["D"], c["ldx"], c["family"], accumulate, res)
            assert ("pool_bmm.onehot" in res) == (c["family"] == "onehot" and not accumulate)
            worst = max(worst, res["pool_bmm"])
    print("worst error / bound", round(worst, 3))


@pytest.mark.parametrize("mutant", pu.BMM_MUTANTS)
def test_bmm_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for c in _bmm_cases():
        for form in ("0", "1"):
            for accumulate in (0, 1):
                if not pu.bmm_applies(mutant, c["family"], form == "1", c["I"], c["J"], c["D"], c["ldx"], accumulate):
                    continue
                res = pu.check_bmm(be, c, accumulate, form)
                assert res["pool_bmm"] >= 4.0, (mutant, c["B"], c["I"], c["J"], c["D"], c["ldx"], c["family"], form, accumulate, res)
                seen += 1
    assert seen >= 100, seen


def _rowdot_cases():
    for B, T, H, D in pu.rowdot_shapes():
        for ldg in (D, D + 4):
            for family in pu.ROWDOT_FAMILIES:
                yield pu.make_rowdot(B, T, H, D, ldg, family)


def test_rowdot_emulation_stays_inside_the_bound():
    be, worst = pu.Emulated(), 0.0
    for n, c in enumerate(_rowdot_cases()):
        res = pu.check_rowdot(be, c, pu.ZERO_N[n % 3])
        assert all(v <= 1.0 for v in res.values()), (c["B"], c["T"], c["H"], c["D"], c["ldg"], c["family"], res)
        worst = max(worst, res["pool_rowdot"])
    print("worst error / bound", round(worst, 3))


@pytest.mark.parametrize("mutant", pu.ROWDOT_MUTANTS)
def test_rowdot_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for c in _rowdot_cases():
        if not pu.rowdot_applies(mutant, c["family"], c["T"], c["D"], c["ldg"]):
            continue
        res = pu.check_rowdot(be, c, 3)
        assert res["pool_rowdot"] >= 4.0, (mutant, c["B"], c["T"], c["H"], c["D"], c["ldg"], c["family"], res)
        seen += 1
    assert seen >= 100, seen


def test_zero_out_rule_rejects_a_wrong_count():
    class Short(pu.Emulated):
        def rowdot(self, gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n):
            return super().rowdot(gmem, ldg, hmem, ds, B, T, H, D, zero_out, max(zero_n - 1, 0))

    class Long(pu.Emulated):
        def rowdot(self, gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n):
            return super().rowdot(gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n + 1)
    c = pu.make_rowdot(1, 1, 1, 4, 4, "normal")
    for zero_n in pu.ZERO_N:
        assert pu.check_rowdot(pu.Emulated(), c, zero_n)["pool_rowdot.zero"] == 0.0
        assert pu.check_rowdot(Long(), c, zero_n)["pool_rowdot.zero"] == pu.INF
        if zero_n:
            assert pu.check_rowdot(Short(), c, zero_n)["pool_rowdot.zero"] == pu.INF
