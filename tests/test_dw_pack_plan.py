"""CPU: nrm_pwattn_bwd_dw_pack reports, without a device, how many consecutive (b,t) groups the fp32 dW_p-only launch reduces together
in whole 4-row steps (bwd_dw_pack_kernel, csrc/pwattn_bwd.hip): P = 4 / gcd(H, 4) where the one-accumulator kernel runs with the blocked
walk and a split holds at least P groups, 1 everywhere else."""
import pytest

KNOBS = ("NRM_DW_PACK", "NRM_DW_DIRECT", "NRM_BT_WAVES", "NRM_BT_INTERLEAVE", "NRM_BT_ORDER")


@pytest.fixture
def ask(lib, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return lambda B, T, H, D, mma=0: lib.nrm_pwattn_bwd_dw_pack(B, T, H, D, mma)


def test_benchmark_shape_packs_pairs(ask):
    assert ask(1024, 30, 50, 400) == 2                      # C3: 126 groups per split, 25 steps per pair instead of 26


def test_groups_that_tile_stay_unpacked(ask):
    assert ask(1024, 30, 128, 768) == 1                     # C5: H % 4 == 0 (and the interleaved walk of big groups)
    assert ask(1024, 30, 48, 400) == 1
    assert ask(2, 4, 16, 80) == 1


def test_odd_heights_pack_quads(ask):
    assert ask(1024, 30, 37, 400) == 4
    assert ask(1024, 30, 17, 64) == 4
    assert ask(1024, 30, 13, 400) == 4                      # the shortest group the one-accumulator kernel takes


def test_short_groups_keep_the_e_form(ask):
    assert ask(1024, 30, 12, 400) == 1                      # three steps per group: bwd_e_kernel serves it
    assert ask(1024, 30, 11, 400) == 1
    assert ask(1024, 30, 5, 400) == 1


def test_split_shorter_than_a_super_group_stays_unpacked(ask, monkeypatch):
    assert ask(2, 3, 50, 400) == 1                          # default plan on a small launch: one group per split
    monkeypatch.setenv("NRM_BT_WAVES", "100")               # 25 tiles: four splits
    assert ask(2, 6, 50, 400) == 2                          # 3 groups per split: a pair and a tail
    assert ask(2, 2, 50, 400) == 1                          # 1 group per split
    assert ask(2, 6, 37, 400) == 1                          # 3 groups per split, quads of 4
    assert ask(2, 8, 37, 400) == 4


def test_knobs_and_other_arithmetics(ask, monkeypatch):
    assert ask(1024, 30, 50, 400, 1) == 1                   # bf16 forms: no one-accumulator kernel
    assert ask(1024, 30, 50, 400, 2) == 1
    monkeypatch.setenv("NRM_DW_PACK", "0")
    assert ask(1024, 30, 50, 400) == 1
    assert ask(1024, 30, 37, 400) == 1
    monkeypatch.setenv("NRM_DW_PACK", "1")
    assert ask(1024, 30, 50, 400) == 2
    assert ask(1024, 30, 128, 768) == 1                     # forcing it on does not make it possible
    monkeypatch.setenv("NRM_DW_DIRECT", "0")
    assert ask(1024, 30, 50, 400) == 1
    monkeypatch.delenv("NRM_DW_DIRECT")
    monkeypatch.setenv("NRM_BT_INTERLEAVE", "1")            # the packed walk is blocked
    assert ask(1024, 30, 50, 400) == 1


def test_bad_arguments(ask):
    assert ask(0, 30, 50, 400) == -1
    assert ask(4, 30, 50, 402) == -1
    assert ask(4, 30, 50, 400, 7) == -1


def test_form_answer_is_unchanged_by_the_packing(lib, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = lib.nrm_pwattn_bwd_form(30, 50, 400, 4, 0, 0)
    assert want == 2 | 4 | 8 | 16                           # one-accumulator family, EXACT, 5x5, writes dW_p: no new bit
    monkeypatch.setenv("NRM_DW_PACK", "0")
    assert lib.nrm_pwattn_bwd_form(30, 50, 400, 4, 0, 0) == want
