"""CPU: the float32 emulation of gemm_nt, gemm_tn and the slab reduction (dense_elements_util.Emulated: fused multiply-add chains in the kernels'
own order, from the memory the kernels are given) inside every bound on every case the GPU test and the worker of tests/dense_knob_worker.py
run; every mutant of the util's docstring rejected -- a ratio above 1, or a broken bitwise / sentinel rule -- by the very ``check_nt`` /
``check_tn`` / ``check_slab`` the GPU test applies, on every case of a shorter list where its ``*_applies`` rule says it can show; G and G' of
the GELU epilogues against the fp32 transcription with exact reciprocal and exp2 (at most HALF of either, the other half is the room of
v_rcp_f32 and v_exp_f32); the mirrors of gemm_nt_select, gemm_tn_plan and slab_plan against the library's host queries; and the case lists
reaching every gemm_nt form the selector can return and all six gemm_tn wave tiles."""
import numpy as np
import pytest

import dense_elements_util as du
import dense_forms_util as dfu


def _ok(res):
    return all(v <= 1.0 for v in res.values())


# ------------------------------------------------------------------------------------------------ GELU
def test_gelu_budgets_hold_the_transcription_to_half():
    """G |z| and G' on 2^16 + 1 points of [-14, 14], +-0 and |z| down to the smallest normal"""
    z = du.gelu_grid()
    assert len(z) >= 2 ** 16 and (np.abs(z) < 2.0 ** -20).sum() >= 4 and 0.0 in z
    assert du.horner_d1() <= du.D1_MAX
    g, gp = du.gelu_grid_ratios()
    print(f"G = {du.G_GELU:.3e}: transcription at {g:.3f} of it;  G' = {du.G_GRAD:.3e}: {gp:.3f}")
    assert g <= 0.5 and gp <= 0.5
    # the statements themselves: gelu' is the derivative of gelu, and the two are those of torch in float64
    import torch
    zz = torch.from_numpy(du.f64(z)).requires_grad_(True)
    y = torch.nn.functional.gelu(zz)
    y.sum().backward()
    assert np.abs(du.gelu64(z) - y.detach().numpy()).max() <= 1e-14 * 14 and np.abs(du.gelu_grad64(z) - zz.grad.numpy()).max() <= 1e-14
    # what the budget is for: the tanh form and a gelu' without x phi(x) are far outside
    assert du.ratio(du.gelu_tanh32(z), du.gelu64(z), du.G_GELU * np.abs(du.f64(z))) > 100
    assert du.ratio(du.gelu_grad32_times(z, np.ones_like(z), without_xphi=True), du.gelu_grad64(z), du.G_GRAD * np.ones(len(z))) > 1000


# ------------------------------------------------------------------------------------------------ the host mirrors
def test_form_mirror_is_the_selector(lib, monkeypatch):
    for k in dfu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert dfu.nt_form(lib, 150, 64, 64) == (4, 1, 4, 1), "run without NRM_NT_SMALLM / NRM_NT_NARROW"
    for NT in du.NT_WIDTHS:
        for M, K, N in du.nt_shapes(NT):
            assert du.lib_nt_form(lib, M, N, K) == du.nt_form(M, N) == (NT, 1, 4, 1), (M, K, N)
    for M, N, form in dfu.LARGE_GRID_CASES:
        assert du.nt_form(M, N) == form
    for NT in du.MT_WIDTHS:
        for M, K, N in du.mt_shapes(NT):
            assert du.nt_form(M, N, small_m=False) == (NT,) + du.NT_PLANNED[NT] + (1,)


def test_case_lists_reach_every_form(lib, monkeypatch):
    """the nine fp32 forms of test_dense_forms_cpu.py (the four with MT > 1 through the worker's list) and the six gemm_tn wave tiles"""
    for k in dfu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("NRM_TN_WAVES", raising=False)
    possible = {dfu.nt_form(lib, M, N, 40) for M in (1, 150, 5000, 200000, 30720) for N in range(1, 2101)}
    reached = {du.nt_form(M, N) for NT in du.NT_WIDTHS for M, K, N in du.nt_shapes(NT)}
    reached |= {du.nt_form(M, N, small_m=False) for NT in du.MT_WIDTHS for M, K, N in du.mt_shapes(NT)}
    assert reached == possible and len(possible) == 9
    assert {du.tn_plan(ni, nj, R)[1:3] for ni, nj, R in du.tn_shapes()} == set(du.TN_SHAPES)


def test_tn_plan_mirror_and_query(lib, monkeypatch):
    splits = set()
    for waves in du.TN_WAVES:
        if waves is None:
            monkeypatch.delenv("NRM_TN_WAVES", raising=False)
        else:
            monkeypatch.setenv("NRM_TN_WAVES", waves)
        for ni, nj, R in du.tn_shapes() + [(402, 1608, 30720), (1608, 402, 2051), (400, 400, 51200), (64, 64, 3840)]:
            plan = du.lib_tn_plan(lib, ni, nj, R)
            assert plan == du.tn_plan(ni, nj, R, waves), (ni, nj, R, waves)
            assert plan[0] == lib.nrm_gemm_tn_nsplit(ni, nj, R, 0) and (plan[0] - 1) * plan[3] < R <= plan[0] * plan[3] and plan[3] % 4 == 0
            if R <= 1001:
                splits.add(plan[0])
    assert {1, 2, 4, 5} <= splits and max(splits) >= 8
    monkeypatch.delenv("NRM_TN_WAVES", raising=False)
    assert lib.nrm_gemm_tn_plan(0, 64, 128, 0, None, None, None) == -1 and lib.nrm_gemm_tn_plan(64, 64, 0, 0, None, None, None) == -1
    assert lib.nrm_gemm_tn_plan(64, 64, 128, 7, None, None, None) == -1 and lib.nrm_gemm_tn_plan(64, 64, 3840, 0, None, None, None) == 30
    # a last split shorter than the others, and a last workgroup with idle waves
    launches = du.tn_launches()
    assert any(c[2] % du.tn_plan(*c[:4])[3] for c in launches) and any(du.tn_plan(*c[:4])[0] % 4 for c in launches)
    assert {c[5] for c in launches} == {0, 3} and {c[6] for c in launches} == {True, False} and {c[7] for c in launches} == {None, 0, 3, 300}


def test_slab_plan_mirror():
    cases = du.slab_cases()
    plans = [s["plan"] for c in cases for s in c["sets"]]
    assert all(spc - 1 + nchunk >= 1 and nchunk >= 1 for _, nchunk, spc in plans) and any(nchunk > 1 for _, nchunk, _ in plans)
    assert du.slab_plan(1920, 64, 64, False)[1:] == (128, 15)          # gemm.hip: a 64 x 64 gradient in 1920 slabs gets 128 chunks of 15
    sets = [s for c in cases for s in c["sets"]]
    assert {s["nsplit"] for s in sets} >= {1, 2, 4, 5, 37} and any(s["prior"].any() for s in sets) and any(not s["prior"].any() for s in sets)
    assert any(s["out2mem"] is not None for s in sets) and any(s["vecmem"] is None for s in sets) and any(c["multi"] and len(c["sets"]) > du.SLAB_MAX for c in cases)


# ------------------------------------------------------------------------------------------------ gemm_nt
def _nt_run(be, launches, form_of):
    for M, K, N, epi, family, variant in launches:
        yield (M, K, N, epi, family, variant), du.check_nt(be, du.nt_case(M, K, N, family), epi, variant, form_of(M, N))


@pytest.mark.parametrize("NT", sorted(du.NT_WIDTHS))
def test_nt_emulation_stays_inside_the_bounds(NT):
    worst = {}
    for tag, res in _nt_run(du.Emulated(), du.nt_launches(du.nt_shapes(NT)), du.nt_form):
        assert _ok(res), (tag, res)
        assert ("nt.onehot" in res) == (tag[3] == "bias" and tag[4] == "onehot" and not tag[5][3])
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 3) for k, v in worst.items()})
    assert len(worst) >= 6


def test_nt_emulation_of_the_planned_forms_stays_inside_the_bounds():
    """the worker's list (NRM_NT_SMALLM=0): several row tiles per wave, blocks of 64 MT rows"""
    n = 0
    for NT in du.MT_WIDTHS:
        launches = du.nt_launches(du.mt_shapes(NT), families=("normal", "scaled", "onehot"))
        for tag, res in _nt_run(du.Emulated(), launches, lambda M, N: du.nt_form(M, N, small_m=False)):
            assert _ok(res), (tag, res)
            n += 1
    assert n == 5 * 5 * 12


MUTANT_SHAPES = ([(M, 42, 3) for M in (1, 17, 65)] + [(65, K, 3) for K in (4, 16, 17, 33)] + [(65, 17, 66), (17, 42, 66), (65, 42, 128), (33, 17, 258),
                 (65, 17, 400), (65, 42, 402)])


@pytest.mark.parametrize("mutant", du.NT_MUTANTS)
def test_nt_mutants_are_rejected_where_they_can_show(mutant):
    be, seen = du.Emulated(mutant), 0
    for M, K, N, epi, family, variant in du.nt_launches(MUTANT_SHAPES):
        c, form = du.nt_case(M, K, N, family), du.nt_form(M, N)
        if not du.nt_applies(mutant, c, epi, variant, form):
            continue
        res = du.check_nt(be, c, epi, variant, form)
        assert not _ok(res), (mutant, M, K, N, epi, family, variant, res)
        seen += 1
    assert seen >= 8, seen


# ------------------------------------------------------------------------------------------------ gemm_tn
def _tn_env(monkeypatch, waves):
    if waves is None:
        monkeypatch.delenv("NRM_TN_WAVES", raising=False)
    else:
        monkeypatch.setenv("NRM_TN_WAVES", waves)


def test_tn_emulation_stays_inside_the_bounds(monkeypatch):
    be, worst = du.Emulated(), {}
    for n, (ni, nj, R, waves, family, dpad, colsum, zero_n) in enumerate(du.tn_launches()):
        _tn_env(monkeypatch, waves)
        res = du.check_tn(be, du.tn_case(ni, nj, R, waves, family, dpad), colsum, zero_n, dws=4 * (n % 2))
        assert _ok(res), (ni, nj, R, waves, family, dpad, colsum, zero_n, res)
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"tn.%dx%d" % s for s in du.TN_SHAPES} | {"tn.colsum"}


@pytest.mark.parametrize("mutant", du.TN_MUTANTS)
def test_tn_mutants_are_rejected_where_they_can_show(monkeypatch, mutant):
    be, seen = du.Emulated(mutant), 0
    for n, (ni, nj, R, waves, family, dpad, colsum, zero_n) in enumerate(du.tn_launches()):
        c = du.tn_case(ni, nj, R, waves, family, dpad)
        if ni == 400 or not du.tn_applies(mutant, c, colsum, zero_n):
            continue
        _tn_env(monkeypatch, waves)
        res = du.check_tn(be, c, colsum, zero_n, dws=4 * (n % 2))
        assert not _ok(res), (mutant, ni, nj, R, waves, family, dpad, colsum, zero_n, res)
        seen += 1
    assert seen >= 8, seen


# ------------------------------------------------------------------------------------------------ slab reduction
@pytest.fixture(scope="module")
def slab_cases():
    return du.slab_cases()


def test_slab_emulation_stays_inside_the_bounds(slab_cases):
    be = du.Emulated()
    for c in slab_cases:
        res = du.check_slab(be, c)
        assert _ok(res), ([(s["nsplit"], s["ni"], s["nj"]) for s in c["sets"]][:3], res)


@pytest.mark.parametrize("mutant", du.SLAB_MUTANTS)
def test_slab_mutants_are_rejected_where_they_can_show(slab_cases, mutant):
    be, seen = du.Emulated(mutant), 0
    for c in slab_cases:
        if not du.slab_applies(mutant, c):
            continue
        res = du.check_slab(be, c)
        assert not _ok(res), (mutant, [(s["nsplit"], s["ni"], s["nj"]) for s in c["sets"]][:3], res)
        seen += 1
    assert seen >= 2, seen
