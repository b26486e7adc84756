"""CPU: the float64 statement of the front end's forward (frontend_forward_util.reference) against the oracle's own
_label_features / _time_features and against a 2-row example worked by hand, the mutants it must be told from, the case lists,
and the argument checks of nrm_frontend_fwd (no device needed: they return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import frontend_forward_util as fu
from oracle import user_model_oracle as orc

INV = "invariant_interest_model."


def _oracle_rows(s, tabs, x):
    """[R, e0 + e1 + e2 + e3] of the oracle's two functions in float64 on the rows x (ids in range, float32-exact scalars)."""
    p = {INV + "category_embedding.0.weight": tabs["cat"], INV + "sentiment_embedding.0.weight": tabs["sen_w"],
         INV + "sentiment_embedding.0.bias": tabs["sen_b"], INV + "type_embedding.0.weight": tabs["type"]}
    for n in ("year", "month", "day", "hour"):
        p[INV + n + "_embedding.0.weight"] = tabs[n]
    p = {k: torch.from_numpy(v.astype(np.float64)) for k, v in p.items()}
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))[None]                    # [1, R, cols]
    c = 4 + s.P
    with orc.precision(torch.float64):
        lab = orc._label_features(p, xt[..., c:c + 1], xt[..., c + 1:c + 1 + s.n_sub], xt[..., c + 1 + s.n_sub:c + 4 + s.n_sub],
                                  xt[..., c + 4 + s.n_sub:c + 5 + s.n_sub])
        tim = orc._time_features(p, xt[..., :4])
    return torch.cat([lab, tim], dim=2)[0].numpy()


def _random_batch():
    s = fu.spec((7, 5, 3, 2), P=6, n_sub=5, behaviour=1, n_cat=23)
    return s, fu.make_tables(s, 11), fu.make_rows(s, 64, False, 12)


def test_reference_matches_the_oracle():
    s, tabs, x = _random_batch()
    ref = fu.reference(s, tabs, x)
    want = _oracle_rows(s, tabs, x)
    assert not ref["flag"]
    assert np.abs(ref["lab"][:, :sum(s.e)] - want).max() <= 1e-12
    assert np.array_equal(ref["lab"][:, sum(s.e):], x[:, fu.need_cols(s) - 2:fu.need_cols(s)].astype(np.float64))
    assert ref["ti"].dtype == np.float32 and np.array_equal(ref["ti"], x[:, 4:4 + s.P])
    assert np.all(ref["S"] >= np.abs(ref["lab"]) - 1e-15)


@pytest.mark.parametrize("mutant", fu.MUTANTS)
def test_the_oracle_tells_the_mutants_apart(mutant):
    s, tabs, x = _random_batch()
    got = fu.reference(s, tabs, x, mutant=mutant)["lab"][:, :sum(s.e)]
    assert np.abs(got - _oracle_rows(s, tabs, x)).max() > 1e-3


def test_reference_by_hand():
    """Two rows, e = (2, 1, 1, 1), two sub-category slots: row 0 repeats id 2, row 1 has a zero (padding) slot, which counts."""
    s = fu.spec((2, 1, 1, 1), P=1, n_sub=2, behaviour=1, n_cat=3, n_type=2, n_time=(2, 2, 2, 2))
    tabs = {"cat": np.array([[1, 2], [10, 20], [100, 200]], dtype=np.float32), "sen_w": np.array([[1, -2, 4]], dtype=np.float32),
            "sen_b": np.array([0.5], dtype=np.float32), "type": np.array([[7], [9]], dtype=np.float32),
            "year": np.array([[1], [2]], dtype=np.float32), "month": np.array([[10], [20]], dtype=np.float32),
            "day": np.array([[100], [200]], dtype=np.float32), "hour": np.array([[1000], [-2000]], dtype=np.float32)}
    #             y  m  d  h  ti    cat sub sub  s0   s1   s2  type read scroll
    x = np.array([[0, 1, 0, 1, 0.25, 1, 2, 2, 1.0, 1.0, 0.5, 1, 3.5, -1.5],
                  [1, 0, 1, 0, -4.0, 2, 0, 1, 1.0, 2.0, 0.25, 0, 0.0, 8.0]], dtype=np.float64)
    ref = fu.reference(s, tabs, x)
    want = np.array([[10 + (100 + 100) / 2, 20 + (200 + 200) / 2, 0.5 + 1 - 2 + 2, 9, 1 + 20 + 100 - 2000, 3.5, -1.5],
                     [100 + (1 + 10) / 2, 200 + (2 + 20) / 2, 0.0, 7, 2 + 10 + 200 + 1000, 0.0, 8.0]])
    assert np.array_equal(ref["lab"], want)                       # (row 1's sentiment: 0.5 + 1 - 4 + 1 = -1.5 -> ReLU 0)
    assert ref["pre"][1, 0] == -1.5
    mags = np.array([[10 + 100, 20 + 200, 0.5 + 1 + 2 + 2, 9, 1 + 20 + 100 + 2000, 3.5, 1.5],
                     [100 + 5.5, 200 + 11, 0.5 + 1 + 4 + 1, 7, 1212, 0.0, 8.0]])
    assert np.array_equal(ref["S"], mags)
    assert list(ref["kind"]) == ["cat", "cat", "sen", "type", "time", "beh", "beh"]
    assert np.array_equal(ref["ti"], np.array([[0.25], [-4.0]], dtype=np.float32)) and not ref["flag"]


def test_reference_truncates_and_clamps():
    s = fu.spec((2, 1, 1, 1), P=1, n_sub=1, behaviour=0)
    tabs = fu.make_tables(s, 3)
    x = fu.make_rows(s, 4, True, 4)
    base = fu.reference(s, tabs, x)
    for c, lim in fu.id_cols(s):
        k = x[:, c].copy()
        y = x.copy()
        y[:, c] = k + 0.999999                                    # .long() truncates
        r = fu.reference(s, tabs, y)
        assert np.array_equal(r["lab"], base["lab"]) and not r["flag"]
        y[:, c] = np.where(k == 0, -0.5, k)                       # trunc(-0.5) = 0: in range
        r = fu.reference(s, tabs, y)
        assert np.array_equal(r["lab"], base["lab"]) and not r["flag"]
        for bad, clamped in ((lim, lim - 1), (-1, 0), (1e9, lim - 1)):
            y[:, c] = bad
            z = x.copy()
            z[:, c] = clamped
            r = fu.reference(s, tabs, y)
            assert r["flag"] and np.array_equal(r["lab"], fu.reference(s, tabs, z)["lab"])


def test_near_zero_sentiment_share_of_the_cases():
    """The float64 reference alone shows how few sentiment elements sit within the rounding bound of the ReLU's kink."""
    worst = 0.0
    for c in fu.all_sweep_cases():
        ref = fu.reference(c.spec, fu.make_tables(c.spec, c.seed), fu.make_rows(c.spec, c.rows, c.f64, c.seed + 1, c.xcols_extra))
        worst = max(worst, fu.near_zero_share(c.spec, ref))
    assert worst < 0.01
    s = fu.spec((3, 4, 1, 1))
    x = fu.make_rows(s, 8, False, 0)
    x[:, 4 + s.P + 1 + s.n_sub:4 + s.P + 4 + s.n_sub] = 0.0       # all-zero scalars: the pre-activation is the bias, 0.05 from 0
    assert fu.near_zero_share(s, fu.reference(s, fu.make_tables(s, 1), x)) == 0.0


def test_case_lists_cover_what_they_name():
    cases = fu.all_sweep_cases()
    assert len(cases) == 48
    assert {fu.width(c.spec) % 4 for c in cases if c.spec.behaviour} == {0, 1, 2, 3}
    assert {fu.width(c.spec) % 4 for c in cases if not c.spec.behaviour} == {0, 1, 2, 3}
    assert any(c.spec.e[1:] == (1, 1, 1) for c in cases)
    for rows in fu.ROWS:                                           # every row-count class meets every value of every knob
        here = [c for c in cases if c.rows == rows]
        assert {c.spec.P for c in here} == set(fu.P_VALUES), rows
        assert {c.spec.n_sub for c in here} == set(fu.NSUB_VALUES), rows
        assert {c.f64 for c in here} == {False, True}, rows
        assert {c.ldlab_extra for c in here} == {0, 8} and {c.ldti_extra for c in here} == {0, 4}, rows
        assert {c.xcols_extra for c in here} == {0, 3}, rows
    assert len({c.seed for c in cases}) == len(cases)


def test_frontend_fwd_validates_on_the_host(lib):
    f = ctypes.c_void_p(0x1000)

    def fwd(x=f, lab=f, err=f, nrows=3, xcols=20, P=4, n_sub=5, beh=1, e=(5, 3, 2, 3), ldlab=16, ldti=4):
        return lib.nrm_frontend_fwd(x, 0, nrows, xcols, P, n_sub, beh, f, 11, e[0], f, f, e[1], f, 5, e[2], f, f, f, f, 7, 13, 6, 4, e[3],
                                    lab, ldlab, f, ldti, err, None)
    for what, kw in {"negative n_sub": dict(n_sub=-1), "17 slots": dict(n_sub=17, xcols=40),
                     "null rows": dict(x=None), "null output": dict(lab=None), "null flag": dict(err=None), "negative rows": dict(nrows=-1),
                     "P = 0": dict(P=0), "e1 = 0": dict(e=(5, 0, 2, 3)), "rows too narrow": dict(xcols=19), "ldlab < width": dict(ldlab=14),
                     "ldti < P": dict(ldti=3)}.items():
        assert fwd(**kw) == -1, what                                  # NRM_EINVAL
        assert lib.nrm_last_error().startswith(b"nrm_frontend_fwd"), (what, lib.nrm_last_error())
    assert fwd(n_sub=17, xcols=40) == -1 and b"n_sub=17 (<= 16 sub-category slots)" in lib.nrm_last_error()
    assert fwd(nrows=0) == 0                                          # nothing to do: no launch
