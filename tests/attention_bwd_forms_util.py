"""What the launches of the pointwise attention's backward run, and the case lists of the GPU tests that have to reach every form of them.

nrm_pwattn_bwd_plan (include/nrm_hotpath.h) answers, without a kernel launch, with the host function each launch itself switches on: the
dz pass (csrc/pwattn_bwd.hip bwd_dz_select), one contraction pass (csrc/capi.hip bwd_pass -> bwd_e_plan, bwd_e_select, bwd_e_walk), the
fp32 dP walk (csrc/pwattn_bwd_dp.hip pwattn_bwd_dp_select) and the resident-W backward of the bf16 arithmetics (csrc/pwattn_bwd_rw.hip
pwattn_bwd_rw_select).  ``launches`` restates which of them ops._attn_bwd_contract makes for one backward.
tests/test_gpu_attention_bwd_forms.py and its child tests/attention_bwd_knob_worker.py take their cases from here and assert the forms with
the query; tests/test_attention_bwd_forms_cpu.py holds the set these lists reach equal to the set the selectors can return and checks
that the walks of several groups per wave are covered at their edges.  Shapes are (B, T, H, D)."""
import json
import os
import sys

F32, BF16, BF16X3 = 0, 1, 2
MMA_BY_NAME = {"f32": F32, "bf16": BF16, "bf16x3": BF16X3}
NAME_OF_MMA = {v: k for k, v in MMA_BY_NAME.items()}
DZ, CONTRACT, DP, RW = 0, 1, 2, 3                           # NRM_BWD_LAUNCH_*
DZ_F32, DZ_HL4 = 0, 1
E_FAMILIES = ("serial", "pipe", "dw_direct", "dw_r32")
FIELDS = {                                                  # out[NRM_PWATTN_BWD_PLAN_LEN] of nrm_pwattn_bwd_plan per launch, in order
    DZ: ("valid", "family", "threads", "rows_class", "slab_cols", "slabs", "hchunk", "nhc", "big_lds", "narrowed", "dz_format"),
    CONTRACT: ("valid", "family", "tile", "exact", "mma", "with_dw", "with_dt", "hl4", "pack", "interleave", "order", "nkw", "ndcol", "nsplit",
               "gps", "last_groups", "last_live", "G"),
    DP: ("valid", "NT", "nchunks", "kchunks", "steps", "grid", "max_steps", "max_items"),
    RW: ("valid", "NG", "mma", "exact", "nks", "workgroups", "waves", "tsplit", "tasks", "rounds", "plain_dh"),
}
PLAN_LEN = 18
LATCHED = ("NRM_BWD_RW", "NRM_DZ_NARROW")                   # read once per process
PER_LAUNCH = ("NRM_BWD_DP", "NRM_DP_GRID", "NRM_DZ_ROWS", "NRM_BH_PIPE", "NRM_DW_DIRECT", "NRM_DW_R32", "NRM_DW_PACK", "NRM_BT_WAVES",
              "NRM_BH_WAVES", "NRM_BT_INTERLEAVE", "NRM_BT_ORDER", "NRM_BRW_WAVES", "NRM_BRW_TSPLIT")
KNOBS = LATCHED + PER_LAUNCH
# the latched settings that select forms the default dispatch never takes: one child process each
LATCHED_SETTINGS = {"rw0": {"NRM_BWD_RW": "0"}, "narrow0": {"NRM_DZ_NARROW": "0"}}
DP_MIN_ELEMS = 100_000_000                                  # ops.DP_MIN_ELEMS (tests/test_attention_bwd_forms_cpu.py holds them equal)
KIND = {DZ: "dz", CONTRACT: "contract", DP: "dp", RW: "rw"}


def declare(lib):
    import ctypes
    lib.nrm_pwattn_bwd_plan.restype = ctypes.c_int
    lib.nrm_pwattn_bwd_plan.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)]
    return lib


_buf = None


def raw(lib, launch, B, T, H, D, pass_=0, mma=F32, dz_format=DZ_F32, cus=256):
    """out[] of nrm_pwattn_bwd_plan as a list, or None where the entry refuses the arguments."""
    global _buf
    if _buf is None:
        import ctypes
        _buf = (ctypes.c_int * PLAN_LEN)()
    rc = lib.nrm_pwattn_bwd_plan(launch, B, T, H, D, pass_, mma, dz_format, cus, _buf)
    if rc != 0:
        assert rc == -1, rc
        return None
    return _buf[:]


def as_form(launch, pass_, v):
    f = dict(zip(FIELDS[launch], v))
    f["launch"], f["pass"], f["raw"] = launch, pass_, v
    if launch == CONTRACT and f["valid"]:
        f["family"] = E_FAMILIES[f["family"]]
    return f


def query(lib, launch, B, T, H, D, pass_=0, mma=F32, dz_format=DZ_F32, cus=256):
    """The answer of nrm_pwattn_bwd_plan as a dict over FIELDS[launch] (+ 'launch', 'pass', 'raw'), or None where the entry refuses the arguments."""
    v = raw(lib, launch, B, T, H, D, pass_, mma, dz_format, cus)
    return None if v is None else as_form(launch, pass_, v)


def key_raw(launch, v):
    """What the closure counts as one form of a launch (indices: FIELDS).
    contract: (family, tile, EXACT, mma, with_dw, with_dt, hl4, pack, interleaved and honoured, gps > 1);
    dz: (family, threads, rows class, dz_format, nhc > 1, big LDS, narrowed);  dp: (NT, nchunks > 1, a workgroup walks more than one item);
    rw: (NG, mma, EXACT, nks > 1, tsplit > 1, plain_dh, rounds > 1)."""
    if launch == CONTRACT:
        return ("contract", E_FAMILIES[v[1]], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[14] > 1)
    if launch == DZ:
        return ("dz", v[1], v[2], v[3], v[10], v[7] > 1, v[8], v[9])
    if launch == DP:
        return ("dp", v[1], v[2] > 1, v[7] > 1)
    return ("rw", v[1], v[2], v[3], v[4] > 1, v[7] > 1, v[10], v[9] > 1)


def key(f):
    return key_raw(f["launch"], f["raw"])


def launches_raw(lib, shape, mma=F32, rows=True, cus=256):
    """[(launch, pass, out[])] of the launches ops._attn_blocks_bwd / _attn_bwd_contract make for one backward of ``shape`` in arithmetic
    ``mma`` under the current environment: the dz pass, then 'rw' (bf16 arithmetics with a resident-W backward), 'dp' (fp32, both row
    gradients wanted, forced or big enough) or the E-form passes.  ``rows``: the target and history rows want a gradient (else the weights
    alone: the dW_p-only pass).  A launch the entry refuses or has no kernel for is an error here: ops would fail."""
    B, T, H, D = shape
    D = (D + 3) // 4 * 4                                     # (ops pads the feature width to a multiple of 4)
    rw = raw(lib, RW, B, T, H, D, 0, mma, 0, cus) if mma != F32 else None
    rw = rw if rw is not None and rw[0] else None
    out = [(DZ, 0, raw(lib, DZ, B, T, H, D, 0, mma, DZ_HL4 if rw else DZ_F32, cus))]
    contract = lambda p, fmt=DZ_F32: out.append((CONTRACT, p, raw(lib, CONTRACT, B, T, H, D, p, mma, fmt, cus)))          # noqa: E731
    forced = os.environ.get("NRM_BWD_DP")
    dp = None
    if not rw and rows and mma == F32 and forced != "0" and (forced == "1" or B * T * H * D >= DP_MIN_ELEMS):
        dp = raw(lib, DP, B, T, H, D, 0, mma, 0, cus)
        dp = dp if dp is not None and dp[0] else None
    if rw:
        if rows:
            out.append((RW, 0, rw))
        contract(4, DZ_HL4)
    elif dp:
        out.append((DP, 0, dp))
        contract(4)
    else:
        contract(1 if rows else 4)
        if rows:
            contract(2)
    assert all(v is not None and v[0] for _l, _p, v in out), (shape, mma, rows, out)
    return out


def launches(lib, shape, mma=F32, rows=True, cus=256):
    """launches_raw as form dicts."""
    return [as_form(*x) for x in launches_raw(lib, shape, mma, rows, cus)]


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


def tiles(D, mma=F32):
    """Wave tiles of the contraction grid (bwd_e_plan): NRM_BT_WAVES / NRM_BH_WAVES = 4 * tiles gives four splits."""
    n16 = (D + 15) // 16
    t = 5 if mma == F32 and (n16 + 4) // 5 * 5 < (n16 + 3) // 4 * 4 else 4
    return ((n16 + t - 1) // t) ** 2


def resolve(settings, shape, mma, lib=None, cus=256):
    """A case's environment.  NRM_BT_WAVES / NRM_BH_WAVES = 'Nt': N x the wave tiles of the case's width.  NRM_BRW_TSPLIT = 'r2': the
    smallest number of parts for which the busiest wave of the resident-W backward makes exactly two trips on ``cus`` compute units (left
    as it is where there is none: the query then refuses nothing and the case fails on its form)."""
    B, T, H, D = shape
    D = (D + 3) // 4 * 4
    out = {k: (str(int(v[:-1]) * tiles(D, mma)) if v.endswith("t") else v) for k, v in settings.items()}
    if out.get("NRM_BRW_TSPLIT") == "r2":
        out["NRM_BRW_TSPLIT"] = "0"
        for ts in range(1, T + 1):
            with env(dict(out, NRM_BRW_TSPLIT=str(ts))):
                v = raw(lib, RW, B, T, H, D, 0, mma, 0, cus)
            if v is not None and v[0] and v[9] == 2:
                out["NRM_BRW_TSPLIT"] = str(ts)
                break
    return out


# ---------------------------------------------------------------------------------------------- the sweep: what the selectors can return
SWEEP_D = tuple(range(4, 1025, 4))
SWEEP_HT = (1, 4, 5, 15, 16, 17, 20, 21, 28, 29, 32, 33, 50, 200, 300)
SWEEP_B = (1, 3, 512)
# Widths the knob settings are swept at: one of every class a knob can tell apart -- 4x4 / 5x5 tiles, exact and ragged, both sides of D = 64
# (NG), 128 (resident slices) and 256 (the resident-W backward), D % 128 == 0 and not, every N-chunk plan of the dP walk, dz slabs of one
# and of several slabs.  The default environment is swept at every width.
KNOB_D = (4, 16, 60, 64, 68, 72, 80, 100, 128, 132, 200, 208, 256, 260, 320, 324, 400, 420, 768, 1024)
# (environment, which arithmetics, rows wanted or not) -- each knob where it can matter; '4t' / '8t': resolve()
SWEEP_ENVS = [
    ({}, (F32, BF16, BF16X3), (True,), SWEEP_D),
    ({}, (F32, BF16, BF16X3), (False,), KNOB_D),
    ({"NRM_BWD_DP": "1"}, (F32,), (True,), SWEEP_D),
    ({"NRM_BWD_DP": "1", "NRM_DP_GRID": "1"}, (F32,), (True,), KNOB_D),
    ({"NRM_BWD_DP": "1", "NRM_DP_GRID": "7"}, (F32,), (True,), KNOB_D),
    ({"NRM_BWD_DP": "0"}, (F32,), (True,), KNOB_D),
    ({"NRM_DZ_ROWS": "0"}, (F32, BF16X3), "dz", SWEEP_D),
    ({"NRM_DZ_ROWS": "1"}, (F32, BF16X3), "dz", SWEEP_D),
    ({"NRM_BH_PIPE": "0"}, (F32,), (True,), KNOB_D),
    ({"NRM_DW_DIRECT": "0"}, (F32,), (False,), KNOB_D),
    ({"NRM_DW_PACK": "0"}, (F32,), (False,), KNOB_D),
    ({"NRM_DW_R32": "0"}, (BF16, BF16X3), (True,), KNOB_D),
    ({"NRM_BT_INTERLEAVE": "0"}, (F32, BF16, BF16X3), (True, False), KNOB_D),
    ({"NRM_BT_INTERLEAVE": "1"}, (F32, BF16, BF16X3), (True, False), KNOB_D),
] + [
    (dict({"NRM_BT_WAVES": w, "NRM_BH_WAVES": w, "NRM_BWD_DP": "0"}, **more), mmas, rowss, KNOB_D)
    for w in ("4t", "8t")
    for more, mmas, rowss in (({}, (F32, BF16, BF16X3), (True, False)), ({"NRM_BT_INTERLEAVE": "1"}, (F32, BF16, BF16X3), (True, False)),
                              ({"NRM_BT_INTERLEAVE": "1", "NRM_BT_ORDER": "1"}, (F32, BF16, BF16X3), (True, False)),
                              ({"NRM_BH_PIPE": "0"}, (F32,), (True,)), ({"NRM_DW_R32": "0"}, (BF16, BF16X3), (True,)),
                              ({"NRM_DW_DIRECT": "0"}, (F32,), (False,)), ({"NRM_DW_PACK": "0"}, (F32,), (False,)))
] + [
    ({"NRM_BRW_WAVES": w, "NRM_BRW_TSPLIT": ts}, (BF16, BF16X3), "rw", KNOB_D)
    for w in ("1", "3") for ts in ("1", "2", "4", "8")
]


def sweep(lib, cus=256, only=None, kinds=(DZ, CONTRACT, DP, RW)):
    """{key: one (shape, arithmetic, rows, environment) that gives it} over the sweep.  The third entry of a SWEEP_ENVS row: the values of
    ``rows``, or 'dz' / 'rw' where the knobs of the row reach that launch alone.  ``only``: a predicate on (D, mma), ``kinds``: the launches
    counted (the children of the latched settings sweep what their knob can change)."""
    out = {}
    for settings, mmas, rowss, widths in SWEEP_ENVS:
        one = {"dz": DZ, "rw": RW}.get(rowss) if isinstance(rowss, str) else None
        if one is not None and one not in kinds:
            continue
        for D in widths:
            for mma in mmas:
                if only is not None and not only(D, mma):
                    continue
                with env(resolve(settings, (1, 1, 1, D), mma)):
                    for H in SWEEP_HT:
                        # (the dz pass reads T in one bound alone, one impression's z under 2^31 bytes: both ends of the list)
                        for T in (SWEEP_HT if one != DZ else (SWEEP_HT[0], SWEEP_HT[-1])):
                            if T * H * D * 4 >= 1 << 31:
                                continue
                            for B in SWEEP_B:
                                if B * T * H * D > 1 << 33:                # (z of more than 32 GB: no device holds it)
                                    continue
                                for rows in ((True,) if one is not None else rowss):
                                    for launch, _p, v in launches_raw(lib, (B, T, H, D), mma, rows, cus):
                                        if (one is None or launch == one) and launch in kinds:
                                            k = key_raw(launch, v)
                                            if k not in out:
                                                out[k] = ((B, T, H, D), mma, rows, settings)
    return out


# ---------------------------------------------------------------------------------------------- cases
# A case is (tag, shape, arithmetic, rows, environment): one backward through ops.pointwise_attention_scores in that arithmetic, with
# (rows) or without a gradient for the target and history rows, under the per-launch knobs of ``environment`` (resolve()).  The tag says
# what the case is in the lists for; ``promise`` checks it against the query, so a case that no longer reaches its form fails.
_SHORT = {"IL": "NRM_BT_INTERLEAVE", "ORD": "NRM_BT_ORDER", "PIPE": "NRM_BH_PIPE", "R32": "NRM_DW_R32", "DIRECT": "NRM_DW_DIRECT",
          "PACK": "NRM_DW_PACK", "ROWS": "NRM_DZ_ROWS", "BRW_WAVES": "NRM_BRW_WAVES", "TSPLIT": "NRM_BRW_TSPLIT"}


def E(waves=None, **knobs):
    """A case's environment: ``waves`` ('4t' / '8t': that many waves per wave tile, i.e. four / eight splits) for both grouped passes, with
    the dP walk off so that the fp32 row gradients come from them; the other knobs by their short names."""
    out = {"NRM_BWD_DP": "0", "NRM_BT_WAVES": waves, "NRM_BH_WAVES": waves} if waves else {}
    out.update({_SHORT[k]: v for k, v in knobs.items()})
    return out


def case_id(case):
    tag, (B, T, H, D), mma, rows, settings = case
    short = {v: k.lower() for k, v in _SHORT.items()}
    knobs = "".join(f"-{short[k]}{v}" for k, v in sorted(settings.items()) if k in short)
    return f"{tag}-{B}x{T}x{H}x{D}-{NAME_OF_MMA[mma]}-{'rows' if rows else 'w'}{'-' + settings['NRM_BT_WAVES'] if 'NRM_BT_WAVES' in settings else ''}{knobs}"


def case_forms(lib, case, cus=256):
    _tag, shape, mma, rows, settings = case
    with env(resolve(settings, shape, mma, lib, cus)):
        return launches(lib, shape, mma, rows, cus)


def promise(case, forms):
    """Why ``forms`` (case_forms) are not what the case's tag says, or None.  'cover': in the lists for the closure alone (its forms at 256
    compute units are what tests/test_attention_bwd_forms_cpu.py counts; the GPU test holds the device's answer equal to them)."""
    tag, (B, T, H, D), mma, _rows, settings = case
    con = [f for f in forms if f["launch"] == CONTRACT]
    bt, bh = [f for f in con if f["pass"] != 2], [f for f in con if f["pass"] == 2]
    rw = [f for f in forms if f["launch"] == RW]
    ok = {
        "cover": lambda: True,
        "pipe": lambda: bh and bh[0]["family"] == "pipe" and bh[0]["gps"] > 1,
        "dt": lambda: bt[0]["gps"] > 1 and (bt[0]["with_dt"] == 1 or (mma != F32 and D <= 256 and bt[0]["hl4"] == 1)),
        "serial_bh": lambda: bh and bh[0]["family"] == "serial" and bh[0]["gps"] > 1,
        "interleave": lambda: bt[0]["interleave"] == 1 and bt[0]["gps"] >= 3 and bt[0]["nsplit"] % 4 != 0,
        "r32": lambda: bt[0]["family"] == "dw_r32" and bt[0]["gps"] > 1,
        "hl4_serial": lambda: bt[0]["family"] == "serial" and bt[0]["hl4"] == 1 and bt[0]["gps"] > 1,
        "rw_rounds": lambda: rw and rw[0]["rounds"] == 2,
        "rw_empty_part": lambda: rw and rw[0]["tsplit"] * -(-T // rw[0]["tsplit"]) >= T + -(-T // rw[0]["tsplit"]),
        "rw_plain": lambda: rw and rw[0]["plain_dh"] == 1,
        "rw_atomic": lambda: rw and rw[0]["plain_dh"] == 0 and rw[0]["nks"] == 1,
        "rw_waves3": lambda: rw and rw[0]["waves"] == 3,
    }[tag]()
    return None if ok else f"{case_id(case)}: the query does not return the form the case is for: {forms}"


# CASES: every one is needed -- without it a form the selectors can return, or an edge of a walk of several groups per wave, is left without
# a GPU case (tests/test_attention_bwd_forms_cpu.py tries each).  Tags:
#   pipe        the pipelined dh kernel with ranges of 3 (one exact 5x5 tile), 3, 3, 3, 1 (ragged 5x5), 2 and 3 on 4x4 tiles, exact and ragged
#   dt          the (b,t) pass with its dt epilogue over several groups per wave (bf16 arithmetics at D <= 256: the dW_p-only pass beside the
#               resident-W backward), four and eight splits
#   hl4_serial  the bf16 arithmetics' dW_p-only pass on the serial kernel (H = 33 > 32 rows)
#   rw_rounds   the resident-W backward with one wave per workgroup and the candidate walk cut (resolve: 'r2') so that the busiest wave makes
#               exactly two trips; rw_empty_part: T = 9 in 4 parts of 3 (the last is empty); rw_plain / rw_atomic: tsplit 1 against 2 at nks = 1
#   cover       the remaining forms at the smallest shape of the search that reaches them
CASES = [
    ("pipe", (1, 21, 9, 64), F32, True, E('4t')),
    ("pipe", (1, 21, 9, 64), F32, True, E('8t')),
    ("pipe", (1, 29, 10, 72), F32, True, E('4t')),
    ("pipe", (1, 29, 10, 72), F32, True, E('8t')),
    ("pipe", (1, 29, 9, 80), F32, True, E('4t')),
    ("pipe", (1, 29, 9, 80), F32, True, E('8t')),
    ("pipe", (3, 21, 5, 100), F32, True, E('4t')),
    ("dt", (2, 7, 5, 320), BF16, True, E('4t')),
    ("dt", (2, 7, 5, 320), BF16, True, E('8t')),
    ("dt", (2, 7, 5, 320), BF16X3, True, E('4t')),
    ("dt", (2, 7, 5, 320), BF16X3, True, E('8t')),
    ("dt", (2, 7, 6, 400), BF16, True, E('4t')),
    ("dt", (2, 7, 6, 400), F32, True, E('8t')),
    ("dt", (2, 9, 7, 100), F32, True, E('4t')),
    ("dt", (2, 9, 7, 100), F32, True, E('8t')),
    ("dt", (3, 6, 5, 64), BF16, True, E('4t')),
    ("dt", (3, 6, 5, 64), BF16, True, E('8t')),
    ("dt", (3, 6, 5, 64), F32, True, E('4t')),
    ("dt", (3, 7, 5, 80), BF16, True, E('4t')),
    ("dt", (3, 7, 5, 80), BF16, True, E('8t')),
    ("dt", (3, 7, 5, 80), BF16X3, True, E('4t')),
    ("dt", (3, 7, 5, 80), F32, True, E('4t')),
    ("interleave", (3, 7, 5, 72), F32, True, E('8t', IL='1')),
    ("hl4_serial", (3, 7, 33, 100), BF16, True, E('4t')),
    ("hl4_serial", (3, 7, 33, 100), BF16X3, True, E('4t')),
    ("rw_rounds", (3, 24, 50, 256), BF16, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (3, 24, 50, 256), BF16X3, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (5, 24, 100, 100), BF16, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (5, 24, 100, 100), BF16X3, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (5, 24, 100, 64), BF16, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (5, 24, 100, 64), BF16X3, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (9, 29, 1, 128), BF16, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (9, 29, 1, 128), BF16X3, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (9, 9, 1, 132), BF16, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_rounds", (9, 9, 1, 132), BF16X3, True, E(BRW_WAVES='1', TSPLIT='r2')),
    ("rw_empty_part", (3, 9, 17, 64), BF16, True, E(TSPLIT='4')),
    ("rw_plain", (3, 9, 17, 128), BF16, True, E(TSPLIT='1')),
    ("rw_plain", (3, 9, 17, 128), BF16X3, True, E(TSPLIT='1')),
    ("rw_atomic", (3, 9, 17, 128), BF16, True, E(TSPLIT='2')),
    ("rw_atomic", (3, 9, 17, 128), BF16X3, True, E(TSPLIT='2')),
    ("cover", (1, 1, 1, 260), BF16, False, E('4t', IL='1')),
    ("cover", (1, 1, 1, 260), BF16, False, E()),
    ("cover", (1, 1, 1, 260), BF16, True, E('4t', IL='1')),
    ("cover", (1, 1, 1, 260), BF16X3, False, E('4t', IL='1')),
    ("cover", (1, 1, 1, 260), BF16X3, False, E()),
    ("cover", (1, 1, 1, 320), BF16, False, E('4t', IL='1')),
    ("cover", (1, 1, 1, 320), BF16, False, E()),
    ("cover", (1, 1, 1, 320), BF16, True, E('4t', IL='1')),
    ("cover", (1, 1, 1, 320), BF16X3, False, E('4t', IL='1')),
    ("cover", (1, 1, 1, 320), BF16X3, False, E()),
    ("cover", (1, 1, 1, 4), BF16X3, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 1, 1, 4), F32, False, E('4t', IL='1')),
    ("cover", (1, 1, 1, 64), BF16, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 1, 1, 64), BF16X3, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 1, 1, 72), F32, False, E('4t', IL='1')),
    ("cover", (1, 1, 5, 260), BF16, True, E('4t')),
    ("cover", (1, 1, 5, 260), BF16X3, True, E('4t', IL='1')),
    ("cover", (1, 1, 5, 320), BF16X3, True, E('4t', IL='1')),
    ("cover", (1, 1, 5, 4), F32, True, E('4t', IL='1')),
    ("cover", (1, 1, 5, 64), F32, True, E('4t', IL='1')),
    ("cover", (1, 1, 5, 72), F32, True, E('4t')),
    ("cover", (1, 1, 5, 80), F32, True, E('4t', IL='1')),
    ("cover", (1, 21, 33, 132), BF16, True, E(IL='1')),
    ("cover", (1, 21, 33, 72), BF16, True, E('8t')),
    ("cover", (1, 21, 5, 4), F32, True, E('4t', IL='1')),
    ("cover", (1, 5, 1, 132), BF16, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 5, 1, 256), BF16, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 5, 1, 260), BF16, False, E('4t')),
    ("cover", (1, 5, 1, 260), BF16, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 260), BF16X3, False, E('4t')),
    ("cover", (1, 5, 1, 260), BF16X3, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 260), BF16X3, True, E('4t', IL='1')),
    ("cover", (1, 5, 1, 320), BF16, False, E('4t')),
    ("cover", (1, 5, 1, 320), BF16, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 320), BF16X3, False, E('4t')),
    ("cover", (1, 5, 1, 320), BF16X3, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 4), F32, False, E('4t')),
    ("cover", (1, 5, 1, 4), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 64), BF16X3, True, E('4t', R32='0', IL='1')),
    ("cover", (1, 5, 1, 72), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 72), F32, True, E('4t', IL='1')),
    ("cover", (1, 5, 1, 80), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 1, 80), F32, True, E('4t', IL='1')),
    ("cover", (1, 5, 17, 4), F32, False, E('4t')),
    ("cover", (1, 5, 17, 4), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 17, 72), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 17, 80), F32, False, E('4t', IL='1')),
    ("cover", (1, 5, 50, 4), F32, False, E('4t')),
    ("cover", (1, 5, 50, 64), F32, False, E('4t')),
    ("cover", (1, 5, 50, 72), F32, False, E('4t')),
    ("cover", (1, 5, 50, 80), F32, False, E('4t')),
    ("cover", (33, 1, 128, 128), BF16, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 128, 128), BF16X3, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 128, 4), BF16, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 128, 4), BF16X3, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 128, 72), BF16, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 128, 72), BF16X3, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 17, 132), BF16, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 17, 132), BF16X3, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 17, 256), BF16X3, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (33, 1, 50, 228), BF16X3, True, E('4t', IL='1')),
    ("cover", (33, 1, 50, 228), F32, True, E(IL='1')),
    ("cover", (33, 5, 33, 256), BF16, True, E(BRW_WAVES='1', TSPLIT='1')),
    ("cover", (5, 1, 1, 260), BF16, True, E('4t', IL='1')),
    ("cover", (5, 1, 1, 320), BF16, True, E('4t', IL='1')),
    ("cover", (5, 5, 17, 4), F32, False, E('8t')),
    ("cover", (5, 5, 17, 64), F32, False, E('8t')),
    ("cover", (5, 5, 17, 72), F32, False, E('8t')),
    ("cover", (5, 5, 17, 80), F32, False, E('8t')),
]

# EXTRA_CASES: the same checks at further shapes the walks are pinned at (the closure does not need them: their forms and edges are reached
# above): the benchmark's width D = 400 (25 wave tiles; (2, 29, 7, 400): 14 groups in eight splits of 2, so the last workgroup has two live
# waves), the serial (b,h) pass (NRM_BH_PIPE=0) on the pipelined shapes and at T = 5, the interleaved walk with at least three groups per
# split and a split count that is no multiple of 4, alone and with NRM_BT_ORDER=1, the 32-row kernel and NRM_DW_R32=0, NRM_BRW_WAVES=3.
EXTRA_CASES = [
    ("pipe", (2, 29, 7, 400), F32, True, E('4t')),
    ("pipe", (2, 29, 7, 400), F32, True, E('8t')),
    ("pipe", (3, 21, 5, 100), F32, True, E('8t')),
    ("dt", (2, 7, 5, 320), F32, True, E('4t')),
    ("dt", (2, 7, 5, 320), F32, True, E('8t')),
    ("dt", (2, 7, 6, 400), BF16, True, E('8t')),
    ("dt", (2, 7, 6, 400), BF16X3, True, E('4t')),
    ("dt", (2, 7, 6, 400), BF16X3, True, E('8t')),
    ("dt", (2, 7, 6, 400), F32, True, E('4t')),
    ("dt", (2, 9, 7, 100), BF16, True, E('4t')),
    ("dt", (2, 9, 7, 100), BF16, True, E('8t')),
    ("dt", (2, 9, 7, 100), BF16X3, True, E('4t')),
    ("dt", (2, 9, 7, 100), BF16X3, True, E('8t')),
    ("dt", (3, 6, 5, 64), BF16X3, True, E('4t')),
    ("dt", (3, 6, 5, 64), BF16X3, True, E('8t')),
    ("dt", (3, 6, 5, 64), F32, True, E('8t')),
    ("dt", (3, 7, 5, 72), BF16, True, E('4t')),
    ("dt", (3, 7, 5, 72), BF16, True, E('8t')),
    ("dt", (3, 7, 5, 72), BF16X3, True, E('4t')),
    ("dt", (3, 7, 5, 72), BF16X3, True, E('8t')),
    ("dt", (3, 7, 5, 72), F32, True, E('4t')),
    ("dt", (3, 7, 5, 72), F32, True, E('8t')),
    ("dt", (3, 7, 5, 80), BF16X3, True, E('8t')),
    ("dt", (3, 7, 5, 80), F32, True, E('8t')),
    ("serial_bh", (1, 21, 9, 64), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (1, 29, 10, 72), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (1, 29, 9, 80), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (1, 5, 10, 72), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (1, 5, 9, 64), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (1, 5, 9, 80), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (2, 29, 7, 400), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (2, 5, 7, 400), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (3, 21, 5, 100), F32, True, E('4t', PIPE='0')),
    ("serial_bh", (3, 5, 5, 100), F32, True, E('4t', PIPE='0')),
    ("interleave", (2, 9, 19, 72), F32, False, E('8t', IL='1')),
    ("interleave", (2, 9, 19, 72), F32, False, E('8t', IL='1', ORD='1')),
    ("interleave", (2, 9, 7, 100), F32, True, E('8t', IL='1')),
    ("interleave", (2, 9, 7, 100), F32, True, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 6, 17, 64), F32, False, E('8t', IL='1')),
    ("interleave", (3, 6, 17, 64), F32, False, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 6, 5, 64), F32, True, E('8t', IL='1')),
    ("interleave", (3, 6, 5, 64), F32, True, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 7, 18, 80), F32, False, E('8t', IL='1')),
    ("interleave", (3, 7, 18, 80), F32, False, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 7, 5, 320), BF16, True, E('8t', IL='1')),
    ("interleave", (3, 7, 5, 320), BF16, True, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 7, 5, 320), BF16X3, True, E('8t', IL='1')),
    ("interleave", (3, 7, 5, 320), BF16X3, True, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 7, 5, 72), F32, True, E('8t', IL='1', ORD='1')),
    ("interleave", (3, 7, 5, 80), F32, True, E('8t', IL='1')),
    ("interleave", (3, 7, 5, 80), F32, True, E('8t', IL='1', ORD='1')),
    ("r32", (3, 7, 20, 100), BF16, True, E('4t')),
    ("r32", (3, 7, 20, 100), BF16X3, True, E('4t')),
    ("r32", (3, 7, 20, 64), BF16, True, E('4t')),
    ("r32", (3, 7, 20, 64), BF16X3, True, E('4t')),
    ("hl4_serial", (3, 7, 20, 100), BF16, True, E('4t', R32='0')),
    ("hl4_serial", (3, 7, 20, 100), BF16X3, True, E('4t', R32='0')),
    ("hl4_serial", (3, 7, 20, 64), BF16, True, E('4t', R32='0')),
    ("hl4_serial", (3, 7, 20, 64), BF16X3, True, E('4t', R32='0')),
    ("hl4_serial", (3, 7, 33, 64), BF16, True, E('4t')),
    ("hl4_serial", (3, 7, 33, 64), BF16X3, True, E('4t')),
    ("rw_empty_part", (3, 9, 17, 64), BF16X3, True, E(TSPLIT='4')),
    ("rw_waves3", (3, 9, 17, 100), BF16, True, E(BRW_WAVES='3')),
    ("rw_waves3", (3, 9, 17, 100), BF16X3, True, E(BRW_WAVES='3')),
]

# The forms behind latched knobs, run by tests/attention_bwd_knob_worker.py in a child process each: {setting: cases}.  KNOB_CASES are needed
# by the closure; KNOB_WIDTH_CASES pin the knob at a shape (NRM_BWD_RW=0 sends the bf16 arithmetics at D <= 256 through the E-form passes,
# whose forms the widths above 256 reach as well).
KNOB_CASES = {
    "rw0": [],
    "narrow0": [("cover", (2, 3, 200, 72), F32, True, E())],          # one 72-column slab of 200 rows: 66 KB of dynamic LDS
}
KNOB_WIDTH_CASES = {
    "rw0": [("dt", s, m, True, E("4t")) for m in (BF16X3, BF16) for s in ((2, 30, 32, 256), (3, 7, 19, 72))],
    "narrow0": [("cover", (2, 15, 200, 64), F32, True, E())],
}
# what each latched setting changes: (a predicate on (D, arithmetic), the launches) its child sweeps
LATCHED_SWEEP = {"rw0": (lambda D, mma: mma != F32 and D <= 256, (CONTRACT, DZ)), "narrow0": (lambda D, mma: mma == F32, (DZ,))}

# Forms the selectors can return that no GPU case launches, each with its reason.  Only shapes that cannot be made small qualify.
NOT_RUN = {}


def walk_features(f):
    """The edges of a walk of several groups per wave that a contract form's case covers: a short last split, a last workgroup with fewer
    than four live waves, and -- the pipelined kernel, whose loop takes two groups per trip -- ranges of an odd and of an even number."""
    out = set()
    if f["launch"] != CONTRACT or f["gps"] <= 1:
        return out
    k = key(f)
    if f["last_groups"] != f["gps"]:
        out.add((k, "short last split"))
    if f["last_live"] < 4:
        out.add((k, "partial last workgroup"))
    if f["family"] == "pipe":
        for n in {f["gps"], f["last_groups"]}:
            if n > 1:
                out.add((k, "odd range" if n % 2 else "even range"))
    return out


def required_walk_features(keys):
    out = set()
    for k in keys:
        if k[0] == "contract" and k[-1]:
            out |= {(k, "short last split"), (k, "partial last workgroup")}
            if k[1] == "pipe":
                out |= {(k, "odd range"), (k, "even range")}
    return out


def reached(lib, cases, cus=256, skip=None):
    """({key: case name}, {walk feature: case name}) over ``cases``; ``skip``: one case left out (the sensitivity check)."""
    keys, feats = {}, {}
    for case in cases:
        if case is skip:
            continue
        for f in case_forms(lib, case, cus):
            keys.setdefault(key(f), case)
            for w in walk_features(f):
                feats.setdefault(w, case)
    return keys, feats


def older_cases(lists):
    """The backward launches of the older GPU tests as cases.  ``lists``: {name: list} taken from tests/test_gpu_attention.py and
    tests/test_gpu_dw_pack.py by the caller (this module imports neither: its children load no torch)."""
    out = []
    add = lambda tag, shapes, mmas, rowss, settings: out.extend(          # noqa: E731
        (f"{tag} {s} {NAME_OF_MMA[m]} rows={r} {e}", tuple(s), m, r, e) for s in shapes for m in mmas for r in rowss for e in settings)
    add("scores_and_grads", lists["SHAPES"] + lists["PIPE_RAGGED_SHAPES"] + lists["FUZZ"], (F32,), (True,), ({},))
    add("bf16", lists["BF16_SHAPES"] + lists["BF16_E_EXACT_SHAPES"], (BF16, BF16X3, F32), (True,), ({},))
    add("fuzz_bf16x3", lists["FUZZ_BF16X3"], (BF16X3,), (True,), ({},))
    add("dz_rows", lists["DZ_ROWS_SHAPES"], (F32, BF16X3), (True,), ({"NRM_DZ_ROWS": "0"}, {"NRM_DZ_ROWS": "1"}))
    add("dp", lists["DP_SHAPES"], (F32,), (True,), [{"NRM_BWD_DP": "0"}] + [dict({"NRM_BWD_DP": "1"}, **g) for g in
                                                                          ({}, {"NRM_DP_GRID": "1"}, {"NRM_DP_GRID": "7"})])
    for s, grid in lists["FUZZ_DP"]:
        add("fuzz_dp", [s], (F32,), (True,), ({"NRM_BWD_DP": "1", "NRM_DP_GRID": str(grid)},))
    for rows in (False, True):
        base = {"NRM_BWD_DP": "1"} if rows else {}
        shapes = [s for s in lists["DIRECT_DW_SHAPES"] if not rows or lists["dp_supported"](s)]
        add("direct_dw", shapes, (F32,), (rows,), [dict(base, **e) for e in ({"NRM_DW_DIRECT": "0"}, {"NRM_DW_DIRECT": "1"},
                                                                              {"NRM_DW_DIRECT": "1", "NRM_BT_INTERLEAVE": "0"},
                                                                              {"NRM_DW_DIRECT": "1", "NRM_BT_INTERLEAVE": "1"})])
    add("batch32", lists["BATCH32_SHAPES"], (F32, BF16X3), (True,), ({},))
    for four in (False, True):
        w = {"NRM_BT_WAVES": "4t"} if four else {}
        add("dw_pack", lists["DW_PACK_SHAPES"], (F32,), (False,), [dict(w, **e) for e in ({"NRM_DW_PACK": "1"}, {"NRM_DW_PACK": "0"},
                                                                                         {"NRM_DW_PACK": "0", "NRM_DW_DIRECT": "0"})])
    add("dw_pack_dp", [(2, 6, 50, 400)], (F32,), (True,), [dict({"NRM_BT_WAVES": "4t", "NRM_BWD_DP": "1"}, **e) for e in
                                                         ({"NRM_DW_PACK": "1"}, {"NRM_DW_PACK": "0"}, {"NRM_DW_PACK": "0", "NRM_DW_DIRECT": "0"})])
    return out


def interleave_waves(lib, shape, mma, cus=256):
    """The NRM_BT_WAVES with which the (b,t)-grouped launch of ``shape`` walks several groups per split the way the interleaved-walk test
    of tests/test_gpu_attention.py wants them: the fewest splits with at least three groups each and a split count that is no multiple of 4
    (a last workgroup with fewer than four live waves); failing that (fewer than 9 groups) any plan with more than one group per split;
    None where there is none."""
    B, T, H, D = shape
    D = (D + 3) // 4 * 4
    fallback = None
    for ns in range(4, B * T + 4, 4):
        waves = str(ns * tiles(D, mma))
        with env({"NRM_BT_WAVES": waves, "NRM_BWD_DP": "0"}):
            f = [f for f in launches(lib, shape, mma, True, cus) if f["launch"] == CONTRACT and f["pass"] != 2][0]
        if f["gps"] >= 3 and f["nsplit"] % 4 != 0:
            return waves
        if f["gps"] > 1 and fallback is None:
            fallback = waves
    return fallback


def interleaved_cases(lib, shapes):
    """The forced-plan launches of test_interleaved_group_walk_matches_oracle (tests/test_gpu_attention.py) on ``shapes`` as cases."""
    out = []
    for s in shapes:
        for m in (F32, BF16X3):
            waves = interleave_waves(lib, s, m)
            for e in ({"NRM_BT_INTERLEAVE": "0"}, {"NRM_BT_INTERLEAVE": "1"}, {"NRM_BT_INTERLEAVE": "1", "NRM_BT_ORDER": "1"}):
                out.append((f"interleaved {s} {NAME_OF_MMA[m]} {e}", tuple(s), m, True, dict(e, NRM_BT_WAVES=waves, NRM_BWD_DP="0")))
    return out


def _jsonable(k):
    return [list(x) if isinstance(x, tuple) else x for x in k]


def _key_of_json(k):
    return tuple(tuple(x) if isinstance(x, list) else x for x in k)


# ---------------------------------------------------------------------------------------------- running a case on the GPU
# (shared by tests/test_gpu_attention_bwd_forms.py and tests/attention_bwd_knob_worker.py; torch and the package are imported on use)
BF16_FWD_TOL, BF16_GRAD_TOL = 1e-2, 3e-2     # plain bf16 against the oracle: the bounds tests/test_gpu_attention.py applies to it
# forced walk against the default plan (one group per wave, one round), "the same products in another summation order", per tensor as
# max |difference| / max |default|: the values tests/test_gpu_attention.py and tests/test_gpu_dw_pack.py use for fp32 and bf16x3.  bf16:
# four times the most two runs of the DEFAULT plan differ from each other (their float atomics meet in another order) over the bf16 cases
# of this file: 5.9e-7 measured on an MI355X (run the GPU test with NRM_BWD_FORMS_RECORD set: 'default_spread')
BF16_DEFAULT_SPREAD = 5.9e-7
WALK_TOL = {F32: 2e-5, BF16X3: 1e-4, BF16: 4 * BF16_DEFAULT_SPREAD}


def _rel(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def difference(got, ref):
    """{tensor: max |got - ref| / max |ref|} over the tensors of two results of tests/attention_budget.run_device."""
    return {k: _rel(got[k], ref[k]) for k in ref}


def run_case(lib, case, cus, measure_default_spread=False):
    """One case on the device at hand -> its figures.  The forms are asked at the device's own compute-unit count and must be those the
    closure counts (at 256), and what the tag promises; every gradient is held to the float64 budget (plain bf16: to its bounds against
    float64) and to the same shape under the default plan."""
    import torch
    import attention_budget as ab
    tag, shape, mma, rows, settings = case
    arith = NAME_OF_MMA[mma]
    forms = case_forms(lib, case, cus)
    assert [key(f) for f in forms] == [key(f) for f in case_forms(lib, case, 256)], (case_id(case), cus, forms)
    assert {w for f in forms for w in walk_features(f)} == {w for f in case_forms(lib, case, 256) for w in walk_features(f)}, (case_id(case), cus)
    why = promise(case, forms)
    assert why is None, why
    bcase = ab.get_case(shape)
    with env({}):
        default = ab.run_device(bcase, arith, rowgrads=rows)
        again = ab.run_device(bcase, arith, rowgrads=rows) if measure_default_spread else None
    with env(resolve(settings, shape, mma, lib, cus)):
        got = ab.run_device(bcase, arith, rowgrads=rows)
    figure = {"forms": [_jsonable(key(f)) for f in forms]}
    if mma == BF16:
        r64 = bcase.reference(torch.float64)
        err = {k: _rel(got[k], r64[k]) for k in got}
        figure["bf16"] = err
        print(f"{case_id(case)}: bf16 against float64 " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert all(v < (BF16_FWD_TOL if k == "s" else BF16_GRAD_TOL) for k, v in err.items()), (case_id(case), err)
    else:
        r = ab.ratios(got, bcase, arith, rowgrads=rows)
        figure["budget"] = {f"{p}|{n}": float(v) for (p, n), v in r.items()}
        (piece, norm), ratio, _frac = ab.worst_margin(r, arith)
        print(f"{case_id(case)}: worst budget ratio {ratio:.2f} of {ab.m_of(piece, arith)} ({piece}, {norm})")
        ab.assert_within_budget(got, bcase, arith, rowgrads=rows)
    d = difference(got, default)
    figure["against_default"] = d
    print(f"{case_id(case)}: against the default plan {max(d.values()):.2e} (allowed {WALK_TOL[mma]:.1e})")
    if again is not None:
        figure["default_spread"] = difference(again, default)
        print(f"{case_id(case)}: two runs of the default plan differ by {max(figure['default_spread'].values()):.2e}")
    assert all(v <= WALK_TOL[mma] for v in d.values()), (case_id(case), d)
    return figure


def summary(case, figure):
    """One record line: the worst budget ratio (in units of its piece's own gate as well), or the bf16 errors, and the distance to the default plan."""
    import attention_budget as ab
    out = {"case": case_id(case), "forms": figure["forms"], "against_default": max(figure["against_default"].values())}
    if "budget" in figure:
        k = max(figure["budget"], key=lambda k: figure["budget"][k] / ab.m_of(k.split("|")[0], NAME_OF_MMA[case[2]]))
        out.update(worst=k, ratio=float(f"{figure['budget'][k]:.4g}"), gate=ab.m_of(k.split("|")[0], NAME_OF_MMA[case[2]]))
    else:
        out["bf16"] = {k: float(f"{v:.3g}") for k, v in figure["bf16"].items()}
    if "default_spread" in figure:
        out["default_spread"] = max(figure["default_spread"].values())
    return out


if __name__ == "__main__":
    # child of tests/test_attention_bwd_forms_cpu.py ('sweep i n': a share of the default sweep; else: the environment carries ONE latched
    # setting); no device is touched.  One line of JSON:
    # the forms the sweep of what the setting changes finds, and the forms the setting's cases reach with each case left out in turn
    # (index -1: none left out).  (The library the parent's fixture has loaded and checked, opened directly: importing the package costs
    # more than the sweep.)
    import ctypes
    _lib = declare(ctypes.CDLL(os.environ.get("NRM_HOTPATH_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "news_recommendation_model_amd", "libnrm_hotpath.so")))
    _which = sys.argv[1]
    if _which == "sweep":                                     # default latched knobs: every _n-th width, for the parent to join
        _i, _n = int(sys.argv[2]), int(sys.argv[3])
        print(json.dumps({"which": _which, "possible": [_jsonable(k) for k in sweep(_lib, only=lambda D, mma: D // 4 % _n == _i)]}))
        sys.exit(0)
    _only, _kinds = LATCHED_SWEEP[_which]
    _cases = KNOB_CASES[_which]
    print(json.dumps({"which": _which, "possible": [_jsonable(k) for k in sweep(_lib, only=_only, kinds=_kinds)],
                      "width": [[_jsonable(key(f)) for f in case_forms(_lib, c)] for c in KNOB_WIDTH_CASES[_which]],
                      "reached": {str(i): [_jsonable(k) for k in reached(_lib, _cases, skip=_cases[i] if i >= 0 else None)[0]]
                                  for i in range(-1, len(_cases))}}))
