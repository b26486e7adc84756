"""Which forward kernel of the pointwise attention a launch takes, and the case lists of the GPU tests that have to reach every one of them.

nrm_pwattn_fwd_form (include/nrm_hotpath.h) answers, without a kernel launch, with the selector the launches themselves switch on
(csrc/pwattn_fwd.hip pwattn_fwd_select, csrc/pwattn_fwd_rw.hip pwattn_fwd_rw_select).  tests/test_gpu_attention_fwd_forms.py and its
child tests/attention_fwd_knob_worker.py take their cases from here and assert the form with the query;
tests/test_attention_fwd_forms_cpu.py holds the set these lists reach equal to the set the selector can return, so a form added later
without a GPU case fails on any machine.  Shapes are (B, T, H, D)."""
import json
import os
import sys

F32, BF16, BF16X3 = 0, 1, 2
MMA_BY_NAME = {"f32": F32, "bf16": BF16, "bf16x3": BF16X3}
NAME_OF_MMA = {v: k for k, v in MMA_BY_NAME.items()}
FAMILIES = ("stream", "rw_tile", "walk_bf16", "walk_f32")
FIELDS = ("valid", "family", "NT", "MT", "WPE", "CT", "NW", "NTS", "KCH", "mma", "save_z", "ragged", "nsplit", "tsplit", "workgroups",
          "tasks", "rounds", "nchunks")                     # out[NRM_PWATTN_FWD_FORM_LEN] of nrm_pwattn_fwd_form, in order
LATCHED = ("NRM_FWD_WALK",)                                # read once per process
PER_LAUNCH = ("NRM_FWD_CT", "NRM_FWD_WALK_F32", "NRM_FWD_TSPLIT")
KNOBS = LATCHED + PER_LAUNCH
WAVES = {"stream": 0, "rw_tile": 16, "walk_bf16": 8, "walk_f32": 8}      # waves of a persistent workgroup
# the latched settings that change what the default dispatch takes: one child process each
LATCHED_SETTINGS = {"walk0": {"NRM_FWD_WALK": "0"}}


def query(lib, B, T, H, D, mma=F32, save_z=1, ragged=0, N=0, max_count=0, k_max=0, cus=256):
    """The answer of nrm_pwattn_fwd_form as a dict over FIELDS (family by name), or None where the entry refuses the arguments.
    ragged = 2: ``T`` carries Mt, the number of 16-row score tiles."""
    import ctypes
    out = (ctypes.c_int * len(FIELDS))()
    rc = lib.nrm_pwattn_fwd_form(B, T, H, D, mma, save_z, ragged, N, max_count, k_max, cus, out)
    if rc != 0:
        assert rc == -1, rc
        return None
    f = dict(zip(FIELDS, out))
    f["family"] = FAMILIES[f["family"]]
    return f


def template(f):
    """The template parameters the family is instantiated with."""
    if f["family"] == "stream":
        return (f["NT"], f["MT"], f["WPE"], f["CT"], f["NW"])
    if f["family"] == "walk_bf16":
        return (f["NTS"], f["KCH"])
    return (f["NTS"],)


def key(f):
    """What the closure counts as one form: (family, template parameters, arithmetic, z stored, raggedness, several column slices, a split
    candidate walk, a wave that goes round its persistent loop more than once)."""
    return (f["family"], template(f), f["mma"], f["save_z"], f["ragged"], f["nsplit"] > 1, f["tsplit"] > 1, f["rounds"] > 1)


def dense_query(lib, shape, mma=F32, save_z=1, cus=256):
    B, T, H, D = shape
    return query(lib, B, T, H, (D + 3) // 4 * 4, mma, save_z, 0, cus=cus)      # (ops pads the feature width to a multiple of 4)


def ragged_query(lib, shape, counts, cus=256):
    """nrm_pwattn_fwd_ragged as ops.attend_pool_ragged_fwd calls it: ``counts[b]`` candidates of impression b."""
    B, _T, H, D = shape
    return query(lib, B, 0, H, D, F32, 0, 1, N=sum(counts), max_count=max(counts), cus=cus)


def hragged_tables(H, counts, L):
    """(N, max_count, Mt, k_max, K) of a history plan: impression b keeps K_b = L_b + [L_b < H] rows, its candidates ceil(K_b / 16) tiles each."""
    K = [l + (1 if l < H else 0) for l in L]
    return sum(counts), max(counts), sum(c * ((k + 15) // 16) for c, k in zip(counts, K)), max(K), K


def hragged_query(lib, shape, counts, L, cus=256):
    """nrm_pwattn_fwd_hragged as ops.attend_pool_hragged_fwd calls it: history lengths ``L[b]`` (live rows before the padding)."""
    B, _T, H, D = shape
    N, max_count, Mt, k_max, _K = hragged_tables(H, counts, L)
    return query(lib, B, Mt, 0, D, F32, 0, 2, N=N, max_count=max_count, k_max=k_max, cus=cus)


class env:
    """with env({...}): the per-launch knobs for the queries (and launches) inside; the others are removed."""

    def __init__(self, settings):
        self.settings = settings

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in PER_LAUNCH}
        for k in PER_LAUNCH:
            os.environ.pop(k, None)
        os.environ.update(self.settings)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------- the sweep: what the selector can return
SWEEP_D = tuple(range(4, 801, 4)) + (1024, 2496)
SWEEP_H = (1, 5, 15, 16, 17, 200)
SWEEP_T = (1, 7, 30)
SWEEP_B = (1, 3, 512)
# the per-launch knobs, each where it can matter: the candidate image on the streaming kernel, the fp32 walk switch at its two widths,
# the split of the candidate walk at the widths that walk (3: with T = 7 the last part is short; 15: T = 7 clamps it)
SWEEP_ENVS = [({}, lambda mma, D: True),
              ({"NRM_FWD_CT": "0"}, lambda mma, D: mma == F32), ({"NRM_FWD_CT": "1"}, lambda mma, D: mma == F32),
              ({"NRM_FWD_WALK_F32": "0"}, lambda mma, D: mma == F32 and D in (64, 128)),
              ({"NRM_FWD_WALK_F32": "1"}, lambda mma, D: mma == F32 and D in (64, 128)),
              ({"NRM_FWD_TSPLIT": "3"}, lambda mma, D: D in (64, 128, 256)),
              ({"NRM_FWD_TSPLIT": "3", "NRM_FWD_WALK_F32": "1"}, lambda mma, D: mma == F32 and D == 128)]


def sweep(lib, cus=256):
    """{key: one (B, T, H, D, environment) that gives it} over the sweep; invalid selections and refused arguments are left out.  The
    ragged forms are asked as full lists: N = B T candidates, T each (ragged = 1), histories of H kept rows (ragged = 2)."""
    out = {}
    for settings, applies in SWEEP_ENVS:
        with env(settings):
            for D in SWEEP_D:
                for mma in (F32, BF16, BF16X3):
                    if not applies(mma, D):
                        continue
                    for H in SWEEP_H:
                        for T in SWEEP_T:
                            for B in SWEEP_B:
                                fs = [query(lib, B, T, H, D, mma, z, 0, cus=cus) for z in (0, 1)]
                                if mma == F32:
                                    fs.append(query(lib, B, 0, H, D, mma, 0, 1, N=B * T, max_count=T, cus=cus))
                                    fs.append(query(lib, B, B * T * ((H + 15) // 16), 0, D, mma, 0, 2, N=B * T, max_count=T, k_max=H, cus=cus))
                                for f in fs:
                                    if f and f["valid"] and f["tasks"] > 0:
                                        out.setdefault(key(f), (B, T, H, D, settings))
    return out


# ---------------------------------------------------------------------------------------------- what the older GPU tests launch
# (tests/test_attention_fwd_forms_cpu.py holds these copies equal to the lists of the modules named)
# test_gpu_attention.py SHAPES + PIPE_RAGGED_SHAPES + DP_SHAPES: training forward (z stored), fp32; test_gpu_attention_budget.py runs them
# with NRM_FWD_CT = 0 | 1 and NRM_FWD_WALK_F32 = 0 | 1 as well
OLD_F32_SHAPES = [(2, 30, 50, 400), (2, 30, 32, 256), (2, 15, 200, 64), (2, 20, 10, 256), (1, 64, 128, 768), (3, 7, 19, 72), (1, 1, 1, 64),
                  (5, 1, 3, 64), (1, 3, 1, 128), (7, 5, 37, 100), (2, 9, 21, 320), (1, 5, 17, 388), (1, 4, 9, 420), (2, 5, 7, 66), (3, 2, 4, 5),
                  (1, 3, 300, 64), (2, 2, 520, 8), (3, 21, 5, 100), (3, 29, 7, 72),
                  (1, 4, 16, 420), (5, 1, 16, 64), (9, 3, 23, 132), (2, 11, 16, 400), (33, 2, 17, 208), (4, 6, 50, 256)]
OLD_F32_ENVS = [{}, {"NRM_FWD_CT": "0"}, {"NRM_FWD_CT": "1"}, {"NRM_FWD_WALK_F32": "0"}, {"NRM_FWD_WALK_F32": "1"}]
# test_fp32_walk_forward_matches_oracle_and_tile_form: with and without z, NRM_FWD_WALK_F32 = 0 | 1 | unset
OLD_WALK_SHAPES = [(2, 15, 200, 64), (256, 15, 200, 64), (3, 7, 19, 64), (1, 1, 1, 64), (5, 1, 3, 64), (2, 33, 16, 64), (1, 40, 17, 64),
                   (2, 15, 50, 128), (3, 5, 9, 128)]
# test_compact_candidate_image_is_bit_identical: with and without z, NRM_FWD_CT = 0 | 1
OLD_CT_SHAPES = [(2, 30, 50, 400), (3, 7, 19, 388), (1, 64, 128, 768), (5, 3, 5, 160), (4, 9, 7, 192), (2, 11, 16, 400), (3, 5, 130, 208),
                 (1, 1, 5, 400), (7, 2, 21, 176), (2, 13, 63, 768)]
# test_bf16_mfma_scores_and_grads_match_fp32_oracle (+ the two shapes test_gpu_attention_budget.py adds): bf16x3 and bf16, z stored
OLD_BF16_SHAPES = [(2, 30, 32, 256), (2, 30, 50, 400), (2, 15, 200, 64), (2, 20, 10, 256), (3, 7, 19, 72), (1, 1, 1, 64), (5, 1, 3, 64),
                   (7, 5, 37, 100), (1, 4, 9, 420), (2, 5, 7, 66), (3, 2, 4, 5), (1, 3, 300, 64), (3, 7, 5, 320), (4, 6, 50, 256), (3, 5, 130, 208)]
# test_gpu_compact.py ATTN_CASES: (shape, candidates per impression, environment)
OLD_RAGGED_CASES = [((4, 12, 20, 160), [12, 0, 1, 7], {}), ((4, 9, 7, 160), [9, 1, 0, 5], {}), ((3, 8, 18, 400), [8, 3, 1], {}),
                    ((3, 6, 17, 200), [5, 0, 6], {}), ((5, 14, 40, 64), [14, 0, 1, 9, 3], {}),
                    ((5, 14, 40, 64), [14, 0, 1, 9, 3], {"NRM_FWD_TSPLIT": "3"}), ((3, 10, 24, 128), [10, 1, 4], {"NRM_FWD_WALK_F32": "1"}),
                    ((3, 10, 24, 128), [10, 1, 4], {}), ((3, 7, 9, 72), [2, 7, 0], {}), ((3, 5, 20, 160), [5, 5, 5], {}), ((3, 5, 33, 64), [5, 5, 5], {})]
# test_gpu_history_compact.py ATTN_CASES: (shape, history lengths, candidates per impression or None for T each, environment)
OLD_HRAGGED_CASES = [((4, 12, 40, 160), [40, 0, 17, 5], None, {}), ((4, 9, 7, 160), [7, 0, 3, 6], None, {}), ((3, 8, 18, 400), [18, 1, 16], None, {}),
                     ((3, 6, 17, 200), [17, 4, 15], None, {}), ((5, 14, 40, 64), [40, 0, 1, 16, 33], None, {}),
                     ((5, 14, 40, 64), [40, 0, 1, 16, 33], None, {"NRM_FWD_TSPLIT": "3"}), ((3, 10, 24, 128), [24, 0, 17], None, {"NRM_FWD_WALK_F32": "1"}),
                     ((3, 10, 24, 128), [24, 0, 17], None, {}), ((3, 7, 9, 72), [9, 3, 0], None, {}),
                     ((4, 12, 20, 160), [20, 7, 0, 16], [12, 0, 1, 7], {}), ((5, 14, 40, 64), [33, 40, 0, 16, 1], [14, 0, 1, 9, 3], {}),
                     ((3, 7, 9, 72), [3, 9, 0], [2, 7, 0], {}), ((3, 5, 20, 160), [20, 20, 20], None, {}), ((3, 5, 33, 64), [33, 33, 33], None, {})]


def _add(out, f, what):
    assert f is not None and f["valid"], what
    if f["tasks"] > 0:
        out.setdefault(key(f), what)


def reached_by_older_tests(lib, cus=256):
    """{key: a case that launches it} over the lists above (default latched knobs)."""
    out = {}
    for settings in OLD_F32_ENVS:
        with env(settings):
            for shape in OLD_F32_SHAPES:
                _add(out, dense_query(lib, shape, F32, 1, cus), ("older f32", shape, settings))
    for settings in ({}, {"NRM_FWD_WALK_F32": "0"}, {"NRM_FWD_WALK_F32": "1"}):
        with env(settings):
            for shape in OLD_WALK_SHAPES:
                for z in (0, 1):
                    _add(out, dense_query(lib, shape, F32, z, cus), ("older walk", shape, settings, z))
    for settings in ({"NRM_FWD_CT": "0"}, {"NRM_FWD_CT": "1"}):
        with env(settings):
            for shape in OLD_CT_SHAPES:
                for z in (0, 1):
                    _add(out, dense_query(lib, shape, F32, z, cus), ("older ct", shape, settings, z))
    with env({}):
        for shape in OLD_BF16_SHAPES:
            for mma in (BF16, BF16X3):
                _add(out, dense_query(lib, shape, mma, 1, cus), ("older bf16", shape, mma))
    for shape, counts, settings in OLD_RAGGED_CASES:
        with env(settings):
            _add(out, ragged_query(lib, shape, counts, cus), ("older ragged", shape, counts, settings))
    for shape, L, counts, settings in OLD_HRAGGED_CASES:
        with env(settings):
            _add(out, hragged_query(lib, shape, counts or [shape[1]] * shape[0], L, cus), ("older hragged", shape, L, counts, settings))
    return out


# ---------------------------------------------------------------------------------------------- the new GPU cases
# A case is (shape or shape rule, per-launch environment); its VARIANTS are the launches the GPU test makes on that one set of inputs and
# references: the dense forward in the three arithmetics with and without the z store, the candidate-ragged and the history-ragged
# forward (fp32, no z).  B = 3: counts [T, 1, T - 1] candidates and histories of [H, 1, H - 1] live rows; otherwise full lists.
DENSE_VARIANTS = [("dense", mma, z) for mma in (F32, BF16X3, BF16) for z in (1, 0)]
ALL_VARIANTS = DENSE_VARIANTS + [("ragged", F32, 0), ("hragged", F32, 0)]


def lists_of(shape):
    """(candidates per impression, live history rows per impression) of a case's ragged variants."""
    B, T, H, _D = shape
    if B == 3:
        return [T, 1, max(T - 1, 1)], [H, 1, max(H - 1, 1)]
    return [T] * B, [H] * B


def variant_query(lib, shape, variant, cus=256):
    kind, mma, z = variant
    counts, L = lists_of(shape)
    if kind == "dense":
        return dense_query(lib, shape, mma, z, cus)
    if kind == "ragged":
        return ragged_query(lib, shape, counts, cus)
    return hragged_query(lib, shape, counts, L, cus)


def variants_of(lib, shape, settings, variants=ALL_VARIANTS, cus=256):
    """[(variant, form)] of the variants of a case that have a kernel (a bf16 width the resident forms cannot hold has none)."""
    with env(settings):
        out = [(v, variant_query(lib, shape, v, cus)) for v in variants]
    return [(v, f) for v, f in out if f is not None and f["valid"] and f["tasks"] > 0]


# 1. default latches, one round: the forms no older test launches.  (3, 5, 17, D): an impression with neighbours on both sides, H no multiple of
# 16, 255 rows (a partial last tile); D the smallest width of its plan with a ragged last tile where there is one.  Resident tiles NTS = 1 .. 8
# in one slice: D = 4, 20, 36, 52, 68, 84, 100; several slices: 132 (NTS 5), 164 (6), 212 (8, and
# 14 streamed tiles), 260 (bf16x3: 3 slices of 6), 516, 612 and 1024 (bf16 NTS 4 in 16 slices, bf16x3 NTS 2 in 32).  H = 7: the per-row
# candidate image of the ragged streaming forms.  The walks with their candidate walk cut in three (T = 5: parts of 2, 2 and 1).
SMALL_CASES = [((3, 5, 17, D), {}) for D in (4, 20, 36, 52, 68, 84, 100, 132, 212, 260, 516, 1024)] + [
    ((3, 5, 7, 612), {}), ((3, 5, 7, 164), {}), ((3, 5, 17, 64), {}), ((3, 5, 17, 256), {}),
    ((3, 5, 17, 64), {"NRM_FWD_TSPLIT": "3"}), ((3, 5, 17, 256), {"NRM_FWD_TSPLIT": "3"}),
    ((3, 5, 17, 128), {"NRM_FWD_WALK_F32": "1"}), ((3, 5, 17, 128), {"NRM_FWD_TSPLIT": "3", "NRM_FWD_WALK_F32": "1"})]

# 2. the second round of the persistent loops: (name, T, H, D, environment, variants); B is the smallest number of impressions for which
# every variant goes round twice with a partial last round on the device at hand (round2_shape).  H = 125 / 250: a ragged last history tile.
# NRM_FWD_TSPLIT=15 on T = 17 candidates: parts of 2, the ninth holds one candidate and the last six are empty.
ROW_LIMIT = 150000
_BF = [("dense", mma, z) for mma in (BF16X3, BF16) for z in (1, 0)]
_F32_ALL = [("dense", F32, 1), ("dense", F32, 0), ("ragged", F32, 0), ("hragged", F32, 0)]
ROUND2_CASES = [(f"tile-1slice-D{D}", 31, 125, D, {}, ALL_VARIANTS) for D in (12, 28, 44, 60, 76, 92, 124)] + [
    (f"tile-slices-D{D}", 30, 150, D, {}, _BF) for D in (132, 164, 196)] + [
    ("tile-slices-D484", 11, 50, 484, {}, [("dense", BF16X3, 1), ("dense", BF16X3, 0)]),
    ("tile-slices-D612", 11, 50, 612, {}, [("dense", BF16X3, 1), ("dense", BF16X3, 0)]),
    ("tile-slices-D1024", 7, 50, 1024, {}, _BF)] + [
    (f"walk-bf16-D{D}", 2, 250, D, {}, _BF) for D in (64, 128, 256)] + [
    (f"walk-bf16-D{D}-tsplit", 17, 250, D, {"NRM_FWD_TSPLIT": "15"}, _BF) for D in (64, 128, 256)] + [
    ("walk-f32-D64", 1, 250, 64, {}, _F32_ALL),
    ("walk-f32-D64-tsplit", 17, 250, 64, {"NRM_FWD_TSPLIT": "15"}, _F32_ALL),
    ("walk-f32-D128", 1, 250, 128, {"NRM_FWD_WALK_F32": "1"}, _F32_ALL),
    ("walk-f32-D128-tsplit", 17, 250, 128, {"NRM_FWD_TSPLIT": "15", "NRM_FWD_WALK_F32": "1"}, _F32_ALL)]


def second_round_ok(f):
    """At least two rounds, and the last one partial: some waves have a task more than others."""
    per_round = f["workgroups"] // max(f["nsplit"], 1) * WAVES[f["family"]]
    return f["rounds"] >= 2 and per_round > 0 and f["tasks"] % per_round != 0


_round2_shapes = {}


def round2_shape(lib, case, cus):
    """(B, T, H, D) of a ROUND2_CASES entry on a device of ``cus`` compute units, or None where no shape under ROW_LIMIT rows has two rounds."""
    name, T, H, D, settings, variants = case
    if (name, cus) not in _round2_shapes:               # (the latched knobs do not change within a process)
        _round2_shapes[(name, cus)] = None
        for B in range(1, ROW_LIMIT // (T * H) + 1):
            fs = variants_of(lib, (B, T, H, D), settings, variants, cus)
            if len(fs) == len(variants) and all(second_round_ok(f) for _v, f in fs):
                _round2_shapes[(name, cus)] = (B, T, H, D)
                break
    return _round2_shapes[(name, cus)]


# 3. the forms behind latched knobs: {setting: [(shape, variants)]} (one round) and {setting: [second-round cases]}, run by
# tests/attention_fwd_knob_worker.py in a child process each.  walk0 has none: every form it selects runs by default at another width.
KNOB_CASES = {
    "walk0": [],
}
KNOB_ROUND2 = {}
# Cases that pin a knob's behaviour at a width rather than a form of their own (the closure does not need them: the same instantiations run
# at other widths).  walk0:
# the tile-by-tile resident kernel at exactly the widths the bf16 walks shadow, compared with the walks' own scores.
KNOB_WIDTH_CASES = {
    "walk0": [((3, 5, 17, D), _BF) for D in (64, 128, 256)],
}

# Forms the selector can return that no GPU case launches, each with its reason.  Only shapes that cannot be made small qualify.
NOT_RUN = {}


def reached_by_new_tests(lib, cus=256, skip=None):
    """{key: case} over SMALL_CASES and ROUND2_CASES (default latched knobs); ``skip``: one case left out (the sensitivity check)."""
    out = {}
    for case in SMALL_CASES:
        if case is skip:
            continue
        for v, f in variants_of(lib, case[0], case[1], cus=cus):
            out.setdefault(key(f), ("small", case, v))
    for case in ROUND2_CASES:
        if case is skip:
            continue
        shape = round2_shape(lib, case, cus)
        assert shape is not None, f"{case[0]}: no shape under {ROW_LIMIT} rows has two rounds on {cus} compute units"
        for v, f in variants_of(lib, shape, case[4], case[5], cus):
            out.setdefault(key(f), ("round2", case[0], v))
    return out


def knob_reached(lib, which, cus=256, skip=None):
    """{key: case} over KNOB_CASES and KNOB_ROUND2 of one latched setting, evaluated in THIS process (the child's, for its latch)."""
    out = {}
    for case in KNOB_CASES[which]:
        if case is not skip:
            for v, f in variants_of(lib, case[0], {}, case[1], cus):
                out.setdefault(key(f), (which, case[0], v))
    for case in KNOB_ROUND2.get(which, []):
        if case is not skip:
            shape = round2_shape(lib, case, cus)
            assert shape is not None, f"{case[0]}: no shape under {ROW_LIMIT} rows has two rounds on {cus} compute units"
            for v, f in variants_of(lib, shape, case[4], case[5], cus):
                out.setdefault(key(f), (which, case[0], v))
    return out


# ---------------------------------------------------------------------------------------------- running a case on the GPU
# (shared by tests/test_gpu_attention_fwd_forms.py and tests/attention_fwd_knob_worker.py; torch and the package are imported on use)
class Data:
    """The seeded 'normal' inputs of tests/attention_budget.py for one shape, on the host and on the device, with the float64 / float32
    oracle scores (and, for the impressions in ``z_of``, pre-activations) evaluated impression by impression: no [B,T,H,4D] tensor of
    more than one impression is formed."""

    def __init__(self, shape, z_of=()):
        import attention_budget as ab
        import torch
        self.shape = tuple(shape)
        B, T, H, D = self.shape
        self.w, self.t, self.h, _g = ab.make_inputs(B, T, H, D)
        self.z_of = tuple(sorted({b % B for b in z_of}))
        self._ref = {}
        self.dev = lambda a: torch.from_numpy(a).cuda()
        self.wd = [self.dev(self.w[k]) for k in ab.WKEYS]

    def reference(self, dtype):
        """(s [B, T, H], {b: z [T, H, D]}) in ``dtype``, as float64 numpy arrays; z = fc1(cat[h, t, t - h, t * h]), the oracle's formula."""
        import numpy as np
        import torch
        from oracle import user_model_oracle as orc
        if dtype not in self._ref:
            B, T, H, D = self.shape
            p = {"a." + k: torch.from_numpy(v).to(dtype) for k, v in self.w.items()}
            s, z = np.empty((B, T, H)), {}
            with torch.no_grad():
                for b in range(B):
                    tb, hb = torch.from_numpy(self.t[b:b + 1]).to(dtype), torch.from_numpy(self.h[b:b + 1]).to(dtype)
                    s[b] = orc.pointwise_attention_scores(p, "a", tb, hb)[0, :, :, 0].double().numpy()
                    if b in self.z_of:
                        te, he = tb[:, :, None, :].expand(1, T, H, D), hb[:, None, :, :].expand(1, T, H, D)
                        feats = torch.cat([he, te, te - he, te * he], dim=-1)
                        z[b] = torch.nn.functional.linear(feats, p["a.mlp.fc1.weight"], p["a.mlp.fc1.bias"])[0].double().numpy()
            self._ref[dtype] = (s, z)
        return self._ref[dtype]

    def emulation(self):
        """(s, {b: z}): bf16x3 scores and pre-activations by the CPU emulation of tests/attention_budget.py (its forward, impression by impression)."""
        import numpy as np
        import torch
        import attention_budget as ab
        if "e3" not in self._ref:
            B, T, H, D = self.shape
            w1, b1 = torch.from_numpy(self.w["mlp.fc1.weight"]), torch.from_numpy(self.w["mlp.fc1.bias"])
            w2, b2 = torch.from_numpy(self.w["mlp.fc2.weight"]).reshape(-1), torch.from_numpy(self.w["mlp.fc2.bias"])
            wh, wt, wd, wp = (w1[:, i * D:(i + 1) * D] for i in range(4))
            s, zs = np.empty((B, T, H)), {}
            for b in range(B):
                t, h = torch.from_numpy(self.t[b]), torch.from_numpy(self.h[b])
                u = ab._product(h, (wh - wd).t(), 3, 0) + b1
                v = ab._product(t, (wt + wd).t(), 3, 0)
                z = ab._product((t[:, None, :] * h[None, :, :]).reshape(T * H, D), wp.t(), 3, 0).reshape(T, H, D) + u[None] + v[:, None]
                s[b] = ((torch.nn.functional.gelu(z) * w2).sum(-1) + b2).double().numpy()
                if b in self.z_of:
                    zs[b] = z.double().numpy()
            self._ref["e3"] = (s, zs)
        return self._ref["e3"]


def launch(data, variant, h=None, t=None):
    """One forward launch of a variant -> ([scores of impression b: [candidates, kept history rows]], z [B, T, H, D] or None).  ``h``, ``t``:
    other history / candidate arrays (the row-containment plants)."""
    import numpy as np
    import torch
    from news_recommendation_model_amd import ops
    from history_compact_util import brute_force_history_plan
    kind, mma, z = variant
    B, T, H, D = data.shape
    hd = data.dev(data.h if h is None else h)
    tsrc = data.t if t is None else t
    if kind == "dense":
        s, zz = ops.pwattn_fwd(data.dev(tsrc), hd, *data.wd, bool(z), mma)
        torch.cuda.synchronize()
        return list(s.cpu().numpy()), (zz if z else None)
    counts, L = lists_of(data.shape)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    i32 = lambda a: data.dev(np.ascontiguousarray(np.asarray(a, dtype=np.int32)))          # noqa: E731
    imp = np.repeat(np.arange(B), counts)
    t_c = data.dev(np.ascontiguousarray(np.concatenate([tsrc[b, :counts[b]] for b in range(B)], axis=0)))
    if kind == "ragged":
        _pooled, s = torch.ops.nrm.attend_pool_ragged_fwd(t_c, hd, *data.wd, i32(imp), i32(off), max(counts), 0)
        torch.cuda.synchronize()
        s = s.cpu().numpy()
        return [s[off[b]:off[b + 1]] for b in range(B)], None
    hp = brute_force_history_plan(counts, L, H)
    K = np.diff(hp["hist_off"])
    hsrc = data.h if h is None else h
    h_c = data.dev(np.ascontiguousarray(np.concatenate([hsrc[b, :K[b]] for b in range(B)], axis=0)))
    tabs = [i32(imp), i32(off), i32(hp["hist_off"])]
    tile_tab = torch.ops.nrm.history_tiles(tabs[0], tabs[1], tabs[2], i32(hp["tile_pre"]), hp["R"], hp["Mt"])
    _pooled, s = torch.ops.nrm.attend_pool_hragged_fwd(t_c, h_c, *data.wd, tabs[0], tabs[1], tabs[2], i32(hp["hist_mult"]), i32(hp["tile_pre"]),
                                                       tile_tab, max(counts), hp["k_max"], 0)
    torch.cuda.synchronize()
    s, out = s.cpu().numpy(), []
    for b in range(B):
        blk = s[16 * hp["tile_pre"][b]:16 * hp["tile_pre"][b + 1]].reshape(counts[b], 16 * ((K[b] + 15) // 16))
        assert not blk[:, K[b]:].any(), ("rows past the kept history are not zero", b)
        out.append(blk[:, :K[b]])
    return out, None


def score_ratios(data, variant, got, impressions=None):
    """{norm: err(got against float64) / yardstick} of the scores, the rule of tests/attention_budget.py for piece 's': one piece per
    impression, the figure is the worst; the yardstick is what the fp32 oracle loses on the same impressions, floored at 2^-23, and for
    bf16x3 no less than what the CPU emulation of bf16x3 loses."""
    import torch
    import attention_budget as ab
    _kind, mma, _z = variant
    bs = range(data.shape[0]) if impressions is None else impressions
    cut = lambda a: [a[b][:got[b].shape[0], :got[b].shape[1]] for b in bs]          # noqa: E731  (the lists of a ragged variant)
    r64 = cut(data.reference(torch.float64)[0])
    e = ab._piece_err("s", [got[b] for b in bs], r64)
    y = ab._piece_err("s", cut(data.reference(torch.float32)[0]), r64)
    if mma == BF16X3:
        y = [max(a, b) for a, b in zip(y, ab._piece_err("s", cut(data.emulation()[0]), r64))]
    return {norm: ev / max(yv, ab.FLOOR) for norm, ev, yv in zip(("max", "l2"), e, y)}


def z_ratios(data, variant, z):
    """The same for the saved pre-activation z = u + v + P W_p^T of the impressions in data.z_of, the fp32 oracle's pre-activation as the
    yardstick (bf16x3: no less than what the CPU emulation of bf16x3 loses, as for the scores)."""
    import torch
    import attention_budget as ab
    r64, r32 = data.reference(torch.float64)[1], data.reference(torch.float32)[1]
    got = [z[b].cpu().numpy() for b in data.z_of]
    e = ab._piece_err("z", got, [r64[b] for b in data.z_of])
    y = ab._piece_err("z", [r32[b] for b in data.z_of], [r64[b] for b in data.z_of])
    if variant[1] == BF16X3:
        e3 = data.emulation()[1]
        y = [max(a, b) for a, b in zip(y, ab._piece_err("z", [e3[b] for b in data.z_of], [r64[b] for b in data.z_of]))]
    return {norm: ev / max(yv, ab.FLOOR) for norm, ev, yv in zip(("max", "l2"), e, y)}


def gate_of(mma):
    import attention_budget as ab
    return {F32: ab.M_F32, BF16X3: ab.M_BF16X3}[mma]


def check_row_plants(data, variant, what):
    """Row containment inside one launch (B = 3): a NaN history row (h = 1 of impression 1), then an Inf candidate row (t = 0 of impression
    1).  The planted row's scores are non-finite, every other score is finite and impressions 0 and 2 stay within the gate.  -> the figures."""
    import numpy as np
    out = {}
    h = data.h.copy()
    h[1, 1, :] = np.nan
    got, _z = launch(data, variant, h=h)
    assert np.isnan(got[1][:, 1]).all(), (what, "the planted history row's scores are not NaN")
    assert np.isfinite(np.delete(got[1], 1, axis=1)).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all(), (what, "NaN left its row")
    out.update({"plant_h|" + k: v for k, v in check_scores(data, variant, got, what + " (NaN row in h)", impressions=(0, 2)).items()})
    t = data.t.copy()
    t[1, 0, :] = np.inf
    got, _z = launch(data, variant, t=t)
    assert not np.isfinite(got[1][0]).any(), (what, "the planted candidate row's scores are finite")
    assert np.isfinite(got[1][1:]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all(), (what, "Inf left its row")
    out.update({"plant_t|" + k: v for k, v in check_scores(data, variant, got, what + " (Inf row in t)", impressions=(0, 2)).items()})
    return out


BF16_BOUND = 1e-2          # plain bf16 is characterised (max |difference| over max |reference|, as tests/test_gpu_attention.py does), not gated


def bf16_error(data, got, impressions=None):
    import numpy as np
    import torch
    bs = range(data.shape[0]) if impressions is None else impressions
    r64 = data.reference(torch.float64)[0]
    return max(np.abs(got[b] - r64[b]).max() for b in bs) / max(np.abs(r64[b]).max() for b in bs)


def check_scores(data, variant, got, what, impressions=None):
    """Print and assert the figure of one launch; -> the figure ({norm: ratio}, or the plain-bf16 relative error)."""
    mma = variant[1]
    if mma == BF16:
        err = bf16_error(data, got, impressions)
        print(f"{what}: bf16 relative error {err:.3e} (bound {BF16_BOUND})")
        assert err < BF16_BOUND, (what, err)
        return {"bf16": float(err)}
    r = score_ratios(data, variant, got, impressions)
    print(f"{what}: s ratios max {r['max']:.2f} l2 {r['l2']:.2f} (M = {gate_of(mma)})")
    assert all(v <= gate_of(mma) for v in r.values()), (what, r)
    return r


def check_plant(data, variant, what):
    """Row containment across rounds: a NaN in history row 0 of impression 0 -- the first tile / task of wave 0 of workgroup 0, the wave that
    also takes the first tile / task of the second round.  Its own scores h = 0 are NaN, every other score of the launch is finite and the
    other impressions stay within the gate."""
    import numpy as np
    B, T, H, D = data.shape
    h = data.h.copy()
    h[0, 0, D // 2] = np.nan
    got, _z = launch(data, variant, h=h)
    assert np.isnan(got[0][:, 0]).all(), (what, "the planted row's scores are not NaN")
    assert np.isfinite(got[0][:, 1:]).all(), (what, "NaN left its history row")
    assert all(np.isfinite(got[b]).all() for b in range(1, B)), (what, "NaN left its impression")
    return check_scores(data, variant, got, what + " (NaN in h[0, 0])", impressions=range(1, B))


def bf16_z_error(data, z):
    import numpy as np
    import torch
    r64 = data.reference(torch.float64)[1]
    return max(np.abs(z[b].cpu().numpy() - r64[b]).max() for b in data.z_of) / max(np.abs(r64[b]).max() for b in data.z_of)


def run_second_round(lib, case, cus):
    """One entry of ROUND2_CASES / KNOB_ROUND2 on the device at hand: every variant is asserted to go round twice with a partial last round,
    its scores are gated per impression against float64, the saved z of the first and the last two impressions (the second round's rows are
    the last ones) likewise, and the launch without a z store is repeated with the NaN plant.  -> (shape, [(variant, form, figures)])"""
    name, _T, _H, _D, settings, wanted = case
    shape = round2_shape(lib, case, cus)
    assert shape is not None, f"{name}: no shape under {ROW_LIMIT} rows gives two rounds on {cus} compute units"
    B = shape[0]
    data = Data(shape, z_of=(0, B - 2, B - 1))
    variants = variants_of(lib, shape, settings, wanted, cus)
    assert len(variants) == len(wanted), (name, shape)
    out = []
    with env(settings):
        for variant, f in variants:
            kind, mma, z = variant
            what = (f"{name} {shape} {kind} {NAME_OF_MMA[mma]} z={z} {f['family']}{template(f)} slices {f['nsplit']} parts {f['tsplit']} "
                    f"tasks {f['tasks']} workgroups {f['workgroups']} rounds {f['rounds']}")
            assert second_round_ok(f), what
            s, zz = launch(data, variant)
            figure = {"s|" + k: v for k, v in check_scores(data, variant, s, what).items()}
            if zz is not None and mma == BF16:
                figure["z|bf16"] = float(bf16_z_error(data, zz))
                print(f"{what}: z bf16 relative error {figure['z|bf16']:.3e} (bound {BF16_BOUND})")
                assert figure["z|bf16"] < BF16_BOUND, what
            elif zz is not None:
                rz = z_ratios(data, variant, zz)
                print(f"{what}: z ratios max {rz['max']:.2f} l2 {rz['l2']:.2f}")
                assert all(v <= gate_of(mma) for v in rz.values()), (what, rz)
                figure.update({"z|" + k: v for k, v in rz.items()})
            if not z:                                             # (one plant per form: the z store does not change who reads which row)
                figure.update({"plant|" + k: v for k, v in check_plant(data, variant, what).items()})
            out.append((variant, f, figure))
    return shape, out


def _jsonable(k):
    return [list(x) if isinstance(x, tuple) else x for x in k]


def _key_of_json(k):
    return tuple(tuple(x) if isinstance(x, list) else x for x in k)


if __name__ == "__main__":
    # child of tests/test_attention_fwd_forms_cpu.py: the environment carries ONE latched setting; no device is touched.  One line of JSON:
    # the forms the sweep finds, and the forms the setting's cases reach with each case left out in turn (index -1: none left out)
    # (the library the parent's fixture has loaded and checked, opened directly: importing the package costs more than the sweep)
    import ctypes
    _lib = ctypes.CDLL(os.environ.get("NRM_HOTPATH_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                       "news_recommendation_model_amd", "libnrm_hotpath.so"))
    _lib.nrm_pwattn_fwd_form.restype = ctypes.c_int
    _lib.nrm_pwattn_fwd_form.argtypes = [ctypes.c_int] * 11 + [ctypes.POINTER(ctypes.c_int)]
    _which = sys.argv[1]
    _cases = KNOB_CASES[_which] + KNOB_ROUND2.get(_which, [])
    print(json.dumps({"which": _which, "possible": [_jsonable(k) for k in sweep(_lib)],
                      "reached": {str(i): [_jsonable(k) for k in knob_reached(_lib, _which, skip=_cases[i] if i >= 0 else None)]
                                  for i in range(-1, len(_cases))}}))
