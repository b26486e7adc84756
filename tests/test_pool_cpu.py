"""CPU: the float64 statements of pool_util against float64 torch.bmm; the float32 fused-multiply-add chain emulation of both pool kernels
-- in j order and in the four quarters of the JSPLIT form -- inside the bound on every case the GPU test runs; and every mutant
rejected at >= 4 x the bound on every case it applies to, by the same ``check_bmm`` / ``check_rowdot`` the GPU test applies.  Second half:
the same for the ragged, history-ragged and weighted entries (``check_ragged`` / ``check_hragged`` / ``check_wlast`` / ``check_rowdot_wlast``):
statements against float64 torch.bmm from the memory the kernel is given, the emulation inside every bound on every case of the GPU test,
fifteen further mutants rejected on every case their ``*_applies`` rule names, and unchanged where the rule says they cannot show."""
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


# ------------------------------------------------------------------------------------------------ the ragged and the weighted forms
def _ragged_cases():
    for order, H, D in pu.ragged_shapes():
        for family in pu.BMM_FAMILIES:
            yield pu.ragged_case(order, H, D, family)
    for family in pu.BMM_FAMILIES:
        for which in (0, 1):
            yield pu.ragged_clamped(family, which)


def _hragged_cases():
    for D in pu.RAGGED_D:
        for family in pu.BMM_FAMILIES:
            yield pu.hragged_case(D, family)
    for family in pu.BMM_FAMILIES:
        yield pu.hragged_clamped(family)


def _wlast_cases(row):
    for I, J, ldx in pu.wlast_shapes(row):
        for layout in (pu.LAYOUTS if row else pu.LAYOUTS[:1]):
            for family in pu.BMM_FAMILIES:
                yield pu.make_wlast(I, J, ldx, layout, family)


def _rowdot_wlast_cases():
    for B, T, H, D, ldg in pu.rowdot_wlast_shapes():
        for family in pu.ROWDOT_FAMILIES:
            yield pu.make_rowdot(B, T, H, D, ldg, family)


def test_ragged_statements_match_float64_bmm_and_the_tables_reach_every_edge():
    for order in (0, 1):
        c = pu.ragged_case(order, 33, 68, "normal")
        assert sorted(rows for _, rows in c["lists"]) == sorted((0, 1, 15, 16, 17, 64, 65, 130, 0)) and c["max_count"] == 130
        assert c["N"] == 311 and c["owned"].sum() == 308 and not c["owned"][308:].any()
        s = torch.from_numpy(np.nan_to_num(c["smem"][:c["N"] * 33])).double().reshape(c["N"], 33)
        h = torch.from_numpy(c["hmem"][:9 * 33 * 68]).double().reshape(9, 33, 68)
        imp = np.repeat(np.arange(9), [rows for _, rows in c["lists"]])
        want = torch.bmm(s[:308, None, :], h[imp])[:, 0].numpy()
        assert np.abs(c["ref"][:308] - want).max() <= 1e-13 * np.abs(want).max()
    assert pu.ragged_case(0, 33, 68, "normal")["lists"][0][1] == 0 and pu.ragged_case(1, 33, 68, "normal")["lists"][-1][1] == 0
    c = pu.hragged_case(68, "normal")
    assert [g["K"] for g in c["lists"]] == list(pu.HRAGGED_K) and [g["written"] for g in c["lists"]] == list(pu.HRAGGED_COUNTS)
    assert c["k_max"] == 65 and c["max_count"] == 130 and c["R"] == sum(pu.HRAGGED_K) and {g["w"] for g in c["lists"]} == {1, 2, 3, 37}
    X = c["hmem"][:c["R"] * 68].reshape(c["R"], 68).astype(np.float64)
    for g in c["lists"]:                                    # the statement, candidate by candidate, from the memory the kernel is given
        for i in range(g["written"]):
            s = c["smem"][16 * (g["t0"] + i * g["nt"]):][:16 * g["nt"]].astype(np.float64)
            assert np.isfinite(s[:g["K"]]).all() and np.isnan(s[g["K"]:]).all()
            wj = np.ones(g["K"])
            wj[-1] = g["w"]
            want = (s[:g["K"]] * wj) @ X[g["r0"]:g["r0"] + g["K"]]
            assert np.abs(c["ref"][g["c0"] + i] - want).max() <= 1e-13 * np.abs(want).max()
    c = pu.hragged_clamped("normal")
    assert [(g["c0"], g["rows"], g["K"], g["written"]) for g in c["lists"]] == [(0, 3, 5, 3), (3, 17, 0, 0), (20, 8, 17, 8), (28, 12, 8, 8), (40, 0, 0, 0)]
    assert np.flatnonzero(c["owned"]).tolist() == [0, 1, 2] + list(range(20, 36))
    assert [pu.ragged_clamped("normal", k)["lists"] for k in (0, 1)] == [[(0, 3), (3, 17), (20, 20), (40, 0)],
                                                                          [(6, 0), (2, 7), (9, 21), (30, 0), (30, 6), (36, 0)]]


def test_weighted_statements_match_float64_bmm():
    for row, (I, J) in ((0, (17, 33)), (1, (65, 5)), (1, (1, 1))):
        c = pu.make_wlast(I, J, 72, "sT" if row else "s", "normal")
        B, D = c["B"], c["D"]
        W = torch.from_numpy(c["wmem"][:B * I * J]).double().as_strided((B, I, J), c["strides"]).clone()
        X = torch.from_numpy(c["xmem"][:B * J * 72]).double().reshape(B, J, 72)[:, :, :D]
        if row:
            want = torch.bmm(W, X)
            want[:, I - 1] *= 37
        else:
            W[:, :, J - 1] *= 37
            want = torch.bmm(W, X)
        for accumulate in (0, 1):
            ref, bound, _ = pu.wlast_bound(c, 37, row, accumulate)
            w = want.numpy() + (c["prior"].astype(np.float64) if accumulate else 0.0)
            assert np.abs(ref - w).max() <= 1e-13 * np.abs(w).max() and np.all(bound > 0)


@pytest.mark.parametrize("form", ["0", "1"])
def test_ragged_emulations_stay_inside_the_bound(form):
    be, worst, ran = pu.Emulated(), {}, 0
    for c in _ragged_cases():
        res = pu.check_ragged(be, c, form)
        assert all(v <= 1.0 for v in res.values()) and ("pool_bmm_ragged.onehot" in res) == (c["family"] == "onehot"), (c["cand_off"], c["H"], c["D"], res)
        worst.update({k: max(v, worst.get(k, 0.0)) for k, v in res.items()})
        ran += 1
    for c in _hragged_cases():
        res = pu.check_hragged(be, c, form)
        assert all(v <= 1.0 for v in res.values()) and ("pool_bmm_hragged.onehot" in res) == (c["family"] == "onehot"), (c["cand_off"], c["D"], res)
        worst.update({k: max(v, worst.get(k, 0.0)) for k, v in res.items()})
        ran += 1
    print("worst error / bound", worst)
    assert ran == 3 * (len(pu.ragged_shapes()) + 2 + len(pu.RAGGED_D) + 1)


@pytest.mark.parametrize("form", ["0", "1"])
def test_weighted_emulations_stay_inside_the_bound(form):
    be, worst, ran = pu.Emulated(), {}, 0
    for row in (0, 1):
        for c in _wlast_cases(row):
            for w in pu.WEIGHTS:
                for accumulate in ((0, 1) if row else (0,)):
                    res = pu.check_wlast(be, c, w, row, accumulate, form)
                    assert all(v <= 1.0 for v in res.values()), (row, c["I"], c["J"], c["ldx"], c["family"], w, accumulate, res)
                    assert (f"pool_bmm_wlast.r{row}.dense_bits" in res) == (w == 1)
                    worst.update({k: max(v, worst.get(k, 0.0)) for k, v in res.items()})
                    ran += 1
    print("worst error / bound", worst)
    assert ran == (len(pu.wlast_shapes(0)) + len(pu.wlast_shapes(1)) * 2 * 2) * 3 * 4


def test_weighted_rowdot_emulation_stays_inside_the_bound():
    be, worst = pu.Emulated(), {}
    for n, c in enumerate(_rowdot_wlast_cases()):
        for w in pu.WEIGHTS:
            res = pu.check_rowdot_wlast(be, c, w, pu.ZERO_N[n % 3])
            assert all(v <= 1.0 for v in res.values()), (c["T"], c["H"], c["D"], c["ldg"], c["family"], w, res)
            worst.update({k: max(v, worst.get(k, 0.0)) for k, v in res.items()})
    print("worst error / bound", worst)
    assert n + 1 == len(pu.rowdot_wlast_shapes()) * 2


@pytest.mark.parametrize("mutant", pu.RAGGED_MUTANTS)
def test_ragged_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for c in _ragged_cases():
        if pu.ragged_applies(mutant, c):
            for form in ("0", "1"):
                res = pu.check_ragged(be, c, form)
                assert res["pool_bmm_ragged"] > 1.0, (mutant, c["cand_off"], c["H"], c["D"], c["family"], form, res)
                seen += 1
    assert seen >= 20, seen


@pytest.mark.parametrize("mutant", pu.HRAGGED_MUTANTS)
def test_hragged_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for c in _hragged_cases():
        for form in ("0", "1"):
            if pu.hragged_applies(mutant, c, pu.jsplit_taken(form, c["B"], c["max_count"], c["k_max"], c["D"])):
                res = pu.check_hragged(be, c, form)
                assert res["pool_bmm_hragged"] > 1.0, (mutant, c["cand_off"], c["D"], c["family"], form, res)
                seen += 1
    assert seen >= (6 if mutant == "tile_clamp_dropped" else 8), seen          # the clamped tables alone / at least every dense case of a form


@pytest.mark.parametrize("mutant", pu.WLAST_MUTANTS)
def test_weighted_bmm_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for row in (0, 1):
        for c in _wlast_cases(row):
            for form in ("0", "1"):
                for w in pu.WEIGHTS:
                    for accumulate in ((0, 1) if row else (0,)):
                        if pu.wlast_applies(mutant, c["family"], form == "1", row, c["I"], c["J"], w, accumulate):
                            res = pu.check_wlast(be, c, w, row, accumulate, form)
                            assert res[f"pool_bmm_wlast.r{row}"] > 1.0, (mutant, row, c["I"], c["J"], c["ldx"], c["family"], form, w, accumulate, res)
                            seen += 1
    assert seen >= 100, seen


@pytest.mark.parametrize("mutant", pu.ROWDOT_WLAST_MUTANTS)
def test_weighted_rowdot_mutants_are_rejected_on_every_case_they_apply_to(mutant):
    be, seen = pu.Emulated(mutant), 0
    for c in _rowdot_wlast_cases():
        for w in pu.WEIGHTS:
            if pu.rowdot_wlast_applies(mutant, c["H"], w):
                res = pu.check_rowdot_wlast(be, c, w, 3)
                assert res["pool_rowdot_wlast"] > 1.0, (mutant, c["T"], c["H"], c["D"], c["ldg"], c["family"], w, res)
                seen += 1
    assert seen >= 100, seen


def test_a_mutant_is_never_run_where_it_cannot_show():
    """the `applies` rules are no blanket: each is False on some case, and there the mutant is indistinguishable from the kernel"""
    c = pu.ragged_clamped("normal", 0)
    assert not pu.ragged_applies("count_not_taken", c)
    assert max(pu.check_ragged(pu.Emulated("count_not_taken"), c, "0").values()) <= 1.0
    assert not pu.wlast_applies("wlast_row_last_of_group", "normal", False, 1, 64, 5, 37, 0)
    c = pu.make_wlast(64, 5, 68, "s", "normal")
    assert max(pu.check_wlast(pu.Emulated("wlast_row_last_of_group"), c, 37, 1, 0, "0").values()) <= 1.0
    assert not pu.rowdot_wlast_applies("rowdot_wlast_last_of_trip", 64, 37)
    c = pu.make_rowdot(2, 17, 64, 20, 24, "normal")
    assert max(pu.check_rowdot_wlast(pu.Emulated("rowdot_wlast_last_of_trip"), c, 37, 0).values()) <= 1.0
    c = pu.hragged_case(68, "normal")
    assert not pu.hragged_applies("tile_clamp_dropped", c, True) and not pu.hragged_applies("mult_in_every_wave", c, False)
    assert max(pu.check_hragged(pu.Emulated("tile_clamp_dropped"), c, "1").values()) <= 1.0
