"""Host side of the table-fed evaluation pass: the runner's plan against ``min`` over each batch restated in numpy, on
the data of the GPU runner test; the numpy restatement of the tally against hand-worked figures; the refusals, which come before any
device call; the new C-ABI symbol and the op, without a GPU."""
import inspect

import numpy as np
import pytest
import torch

from table_scoring_util import B, GUARD, N, plan_reference, scoring_tables, tally_reference


def test_plan_is_the_minimum_of_empty_num_per_batch():
    from news_recommendation_model_amd import evaluation, tables
    _dims, t, T = scoring_tables()
    empty = t.empty_num_all(T, keep_target_slot=False)
    host = tables.assemble_host(t, np.arange(N), 3, T, keep_target_slot=False)
    assert np.array_equal(empty, host["empty_num"])                   # the closed form is what the assembled rows hold
    assert host["label"].sum(axis=1).min() == 1 and (T - empty).min() >= 2      # both classes in every row
    plan = evaluation.scoring_plan(empty, N, B, T)
    assert plan == plan_reference(empty, N, B, T)
    assert [n for n, _ in plan] == [B] * 5 + [3]
    full = [tp for n, tp in plan if n == B]
    # what the GPU test relies on, asserted on the host data so that another seed fails here: more than one width among the full batches,
    # a batch at the full width, and a batch in which some row keeps padding of its own after the common trim
    assert len(set(full)) >= 2 and T in full
    assert any((empty[i * B:(i + 1) * B] - (T - tp)).max() > 0 for i, (n, tp) in enumerate(plan))
    # any order: the plan follows the permuted empty_num
    order = np.random.default_rng(2).permutation(N)
    assert evaluation.scoring_plan(empty[order], N, B, T) == plan_reference(empty[order], N, B, T)
    assert evaluation.scoring_plan(empty, N, N, T) == [(N, T)] and evaluation.scoring_plan(empty[:1], 1, B, T) == [(1, int(T - empty[0]))]
    with pytest.raises(ValueError, match="entries of empty_num"):
        evaluation.scoring_plan(empty[:-1], N, B, T)
    with pytest.raises(ValueError, match="candidate columns"):
        evaluation.scoring_plan(np.full(N, T), N, B, T)               # a batch of empty lists has no width


def test_tally_reference_by_hand():
    """two steps of two rows at T = 3, the second overhanging a pass of three impressions, ring of two rows"""
    f32, i32 = np.float32, np.int32
    steps = [dict(auc=np.array([0.5, -1.0], f32), top1=np.array([1, 0], i32), metrics=np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]], f32),
                  rank=np.array([[2, 1], [1, 0]], i32), live=np.array([2, 1], i32), impression_id=np.array([70, 71], np.int64)),
             dict(auc=np.array([0.25, 0.75], f32), top1=np.array([1, 1], i32), metrics=np.array([[0.5, 0.0, 0.25], [1.0, 1.0, 1.0]], f32),
                  rank=np.array([[1, 2, 3], [3, 2, 1]], i32), live=np.array([3, 3], i32), impression_id=np.array([72, 73], np.int64))]
    got = tally_reference(steps, T=3, n_order=3, cap=2)
    assert got["cursor"] == 4
    assert got["sums"].tolist() == [0.75, 2.0, 1.5, 1.0, 1.25]       # row 3 of the pass (auc 0.75, top1 1, metrics 1) is outside: not summed
    assert got["counts"].tolist() == [1, 1, 2, 3]
    assert got["rec_rank"].tolist() == [[1, 2, 3], [1, 0, 0]]         # position 2 overwrote position 0; position 1 zero-filled; 3 not written
    assert got["rec_live"].tolist() == [3, 1] and got["rec_id"].tolist() == [72, 71]
    none = tally_reference([dict(steps[0], auc=None, top1=None, metrics=None)], T=3, n_order=8, cap=0)
    assert none["sums"].tolist() == [0.0] * 5 and none["counts"].tolist() == [0, 0, 1, 2] and none["rec_id"].shape == (0,)
    untouched = tally_reference(steps[:1], T=3, n_order=8, cap=4)
    assert untouched["rec_id"].tolist() == [70, 71, GUARD, GUARD]


def test_runner_refuses_before_any_device_call(monkeypatch):
    """the arguments are stand-ins, as in test_table_epoch_cpu.py: a refusal that touched a model or a table would fail on them"""
    from news_recommendation_model_amd import evaluation, native, trainer
    G = evaluation.GraphedTableScoring
    sig = inspect.signature(G.__init__).parameters
    assert sig["with_labels"].default is True and sig["record_rows"].default is None and sig["max_graphs"].default == 16
    with pytest.raises(RuntimeError, match="captured step"):
        G([None], None, 8, 17, 5, True, compact=True)
    with pytest.raises(RuntimeError, match="captured step"):
        G([None], None, 8, 17, 5, True, compact_history=True)
    with pytest.raises(RuntimeError, match="1 .. 8"):
        G([None] * 9, None, 8, 17, 5, True)
    with pytest.raises(RuntimeError, match="1 .. 8"):
        G([], None, 8, 17, 5, True)
    with pytest.raises(ValueError, match="batch_size"):
        G([None], None, 0, 17, 5, True)
    monkeypatch.setattr(native, "kernel_events", [])
    with pytest.raises(RuntimeError, match="per-kernel event timing"):
        G([None], None, 8, 17, 5, True)
    monkeypatch.setattr(native, "kernel_events", None)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(RuntimeError, match="process group"):
        G([None], None, 8, 17, 5, True)
    with pytest.raises(RuntimeError, match="process group"):          # the trainer builds the validation runner before the first step
        trainer.train_epochs_tables(None, None, None, 1, 8, 17, 5, validation=object(), validation_graph=True)


def test_entry_points_and_defaults():
    from news_recommendation_model_amd import evaluation, trainer
    sig = inspect.signature(trainer.train_epochs_tables).parameters
    assert sig["validation"].default is None and sig["validation_batch"].default == 80 and sig["validation_graph"].default is None
    for fn, keep in ((evaluation.validate_tables, True), (evaluation.score_tables, False), (evaluation.sweep_checkpoints, True)):
        sig = inspect.signature(fn).parameters
        assert sig["batch_size"].default == 80 and sig["keep_target_slot"].default is keep and "graph" in sig and "H" in sig and "T" in sig


def test_symbol_signature_and_op_are_there(lib):
    from news_recommendation_model_amd import native, ops
    assert "nrm_eval_tally" in native.SIGNATURES and len(native.SIGNATURES["nrm_eval_tally"][1]) == 18
    assert hasattr(lib, "nrm_eval_tally")
    assert "eval_tally" in ops.OPS and ops.eval_tally is torch.ops.nrm.eval_tally
    schema = str(torch.ops.nrm.eval_tally.default._schema)
    for name in ("cursor", "sums", "counts", "rec_rank", "rec_live", "rec_id"):
        assert f"!) {name}" in schema or f"!)? {name}" in schema, schema     # every written argument is annotated as mutated


def test_op_fake_checks_shapes():
    """the fake function runs on meta tensors: the shape and dtype rules hold without a device"""
    from news_recommendation_model_amd import ops
    m = lambda shape, dt: torch.empty(shape, dtype=dt, device="meta")      # noqa: E731
    b, T, tp, cap = 4, 5, 3, 8
    good = dict(auc=m((b,), torch.float32), top1=m((b,), torch.int32), metrics=m((b, 3), torch.float32), rank=m((b, tp), torch.int32),
                live=m((b,), torch.int32), impression_id=m((b,), torch.int64), cursor=m((1,), torch.int64), sums=m((5,), torch.float64),
                counts=m((4,), torch.int64), rec_rank=m((cap, T), torch.int32), rec_live=m((cap,), torch.int32), rec_id=m((cap,), torch.int64),
                n_order=9)
    assert ops.eval_tally(**good) is None
    assert ops.eval_tally(**dict(good, auc=None, top1=None, metrics=None)) is None
    assert ops.eval_tally(**dict(good, rec_rank=None, rec_live=None, rec_id=None)) is None
    for bad in (dict(top1=None), dict(rec_live=None), dict(rec_rank=m((cap, tp - 1), torch.int32)), dict(rec_rank=m((6, T), torch.int32),
                rec_live=m((6,), torch.int32), rec_id=m((6,), torch.int64)), dict(sums=m((3,), torch.float64)), dict(counts=m((2,), torch.int64)),
                dict(rank=m((b, tp), torch.int64)), dict(n_order=-1)):
        with pytest.raises(RuntimeError, match="eval_tally"):
            ops.eval_tally(**dict(good, **bad))
