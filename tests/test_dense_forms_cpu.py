"""CPU: nrm_gemm_nt_form reports, without a device, which gemm_nt_kernel<NT, MT, EPI, WPE> (fp32) or gemm_nt_rx_kernel<RT, MMA, EPI, G>
(bf16 / bf16x3) a launch of nrm_gemm_nt takes -- the selector the launch itself calls (csrc/gemm.hip gemm_nt_select, csrc/gemm_bf16.hip
gemm_nt_rx_select).  The answers for the production layers are pinned, and the set of forms the selector can return is held equal to
the set the GPU cases of tests/dense_forms_util.py reach.  The forms behind the knobs that are latched once per process (NRM_NT_SMALLM,
NRM_NT_NARROW) are enumerated by the child process of tests/test_gpu_dense.py, not here."""
import pytest

import dense_forms_util as dfu
from dense_forms_util import BF16, BF16X3, F32


@pytest.fixture
def forms(lib, monkeypatch):
    for k in dfu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    # the latched knobs were read at the first query of this process: these tests describe the default dispatch
    assert dfu.nt_form(lib, 150, 64, 64) == (4, 1, 4, 1) and dfu.nt_form(lib, 150, 258, 64) == (9, 1, 4, 1), "run without NRM_NT_SMALLM / NRM_NT_NARROW"
    assert dfu.nt_form(lib, 150, 402, 64) == (13, 1, 4, 1)
    return lib


def test_production_layers_fp32(forms):
    nt = lambda M, N, K: dfu.nt_form(forms, M, N, K)                # noqa: E731
    assert nt(30720, 1608, 402) == (13, 1, 4, 1)                    # the head, C3: 13 column tiles x one row tile, four waves per SIMD
    assert nt(30720, 402, 1608) == (13, 1, 4, 1)
    for M in (15360, 5120):                                         # C2 / C1: fewer than 512 workgroups -> one row tile per wave
        assert nt(M, 258, 1032) == (9, 1, 4, 1)
        assert nt(M, 264, 66) == (9, 1, 4, 1)
        assert nt(M, 66, 264) == (5, 1, 4, 1)
    assert nt(51200, 256, 256) == (8, 3, 2, 1)                      # 267 blocks of 192 rows x 2 N-chunks


def test_production_layers_bf16(forms):
    for mma in (BF16, BF16X3):
        assert dfu.rx_form(forms, 15360, 1032, 258, mma) == (4, 3)  # K = 258, nine chunks: 64-row blocks, 240 of them
        assert dfu.rx_form(forms, 15360, 258, 1032, mma) == (2, 3)  # K = 1032, 33 chunks: 32 rows fit half the LDS
        assert dfu.rx_form(forms, 51200, 64, 64, mma) == (8, 3)     # 128-row blocks
    for (M, K, N), want in dfu.BF16_EXPECTED.items():
        for mma, (fwd, dx) in want.items():
            assert dfu.rx_form(forms, M, N, K, mma) == fwd, (M, K, N, mma)
            assert dfu.rx_form(forms, M, K, N, mma) == dx, (M, K, N, mma)


def test_large_grid_cases_take_their_forms(forms):
    for M, N, form in dfu.LARGE_GRID_CASES:
        assert dfu.nt_form(forms, M, N, dfu.LARGE_GRID_K) == form, (M, N)
        assert M % (64 * form[1]) == 1                                 # full blocks and one block of a single row
        assert dfu.nt_form(forms, M // 2, N, dfu.LARGE_GRID_K)[1] == 1  # half the rows: below 512 workgroups, one row tile per wave


# the issue's sweep, and the row counts of the production layers on top (the 64-row bf16 blocks exist only between the M that is
# too small for 200 blocks of 64 rows and the M that is enough for 200 blocks of 128)
SWEEP_M = (1, 150, 5000, 200000, 15360, 30720)
SWEEP_K = (16, 40, 130, 256, 128)               # 128: four chunks (G = 4) whose 128 bf16x3 rows still fit half the LDS; at K = 256 only bf16's do


def test_every_form_the_selector_returns_has_a_gpu_case(forms):
    possible = set()
    for M in SWEEP_M:
        for K in SWEEP_K:
            for N in range(1, 2101):
                possible.add(dfu.dense_form(forms, M, N, K, F32))
            for mma in (BF16, BF16X3):                              # (the bf16 forms do not depend on N)
                possible.add(dfu.dense_form(forms, M, 64, K, mma))
                possible.add(dfu.dense_form(forms, M, 2100, K, mma))
    reached = dfu.reached_forms(forms)
    assert possible - reached == set(), "forms without a GPU case"
    assert reached - possible == set(), "forms the sweep does not find: widen the sweep"
    # what the set is today: 5 planned and 4 one-row-tile fp32 forms, one K-chunk per LDS stage in all of them; RT x G for each bf16 arithmetic
    assert len({f for f in possible if f[0] == "nt"}) == 9 and all(f[4] == 1 for f in possible if f[0] == "nt")
    assert {f[1:] for f in possible if f[0] == "rx"} == {(mma, rt, g) for mma in (BF16, BF16X3) for rt in (1, 2, 4, 8) for g in (3, 4)}


def test_bad_arguments(forms):
    ask = forms.nrm_gemm_nt_form
    assert ask(0, 64, 64, 0) == -1
    assert ask(-5, 64, 64, 0) == -1
    assert ask(64, 0, 64, 0) == -1
    assert ask(64, 64, 0, 1) == -1
    assert ask(64, 64, 64, 3) == -1
    assert ask(64, 64, 64, -1) == -1
    # a reduction width the resident-row form does not take is no error: 0, as nrm_gemm_nt_bf16_supported says
    for mma in (BF16, BF16X3):
        for K in (64, 1608, 4096, 20000, 100000):
            assert (ask(300, 64, K, mma) == 0) == (forms.nrm_gemm_nt_bf16_supported(300, K, mma) == 0), (K, mma)
    assert ask(300, 64, 100000, BF16X3) == 0


def test_knobs_read_at_every_call(forms, monkeypatch):
    assert dfu.rx_form(forms, 51200, 64, 64, BF16) == (8, 3)
    monkeypatch.setenv("NRM_RX_BM", "32")
    assert dfu.rx_form(forms, 51200, 64, 64, BF16) == (2, 3)
