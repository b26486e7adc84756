"""CPU: the scoring tail's C ABI (nrm_ensemble_rank: host-side validation only, nothing is launched), the predictions writer
of reference test.py:76-132 and the registration of torch.ops.nrm.ensemble_rank."""
import ctypes
import os
import zipfile

import numpy as np
import pytest
import torch

from news_recommendation_model_amd import native


def test_abi_7_and_candidate_cap(lib):
    assert lib.nrm_abi_version() == 7 and native.ABI_VERSION == 7
    assert lib.nrm_ensemble_rank_max_candidates() >= 1024


def _call(lib, logits="ok", M=2, T=30, label=None, metrics=None, B=4, outputs=True):
    """nrm_ensemble_rank with never-dereferenced fake device addresses: every case here is refused before a launch."""
    fake = ctypes.c_void_p(0x1000)
    ptrs = (ctypes.c_void_p * 8)(*[0x1000] * 8) if logits == "ok" else logits
    strides = (ctypes.c_long * 8)(*[T] * 8)
    out = fake if outputs else None
    return lib.nrm_ensemble_rank(ptrs, strides, None, M, None, label, B, T, out, out, out, metrics, None)


def test_argument_validation_needs_no_device(lib):
    cap = lib.nrm_ensemble_rank_max_candidates()
    fake = ctypes.c_void_p(0x1000)
    cases = {
        "null logits": dict(logits=None),
        "M = 0": dict(M=0),
        "M = 9": dict(M=9),
        "T = 0": dict(T=0),
        "T = cap + 1": dict(T=cap + 1),
        "label without metrics": dict(label=fake, metrics=None),
        "metrics without label": dict(label=None, metrics=fake),
        "null outputs": dict(outputs=False),
        "negative B": dict(B=-1),
    }
    for what, kw in cases.items():
        rc = _call(lib, **kw)
        assert rc != 0, what
        msg = lib.nrm_last_error()
        assert msg.startswith(b"nrm_ensemble_rank") and len(msg) > 20, (what, msg)
    _call(lib, T=cap + 1)
    assert str(cap).encode() in lib.nrm_last_error()                       # the message names the cap
    null_entry = (ctypes.c_void_p * 8)(0x1000, None)
    assert _call(lib, logits=null_entry) != 0 and b"logits[1]" in lib.nrm_last_error()
    assert _call(lib, B=0) == 0                                            # an empty batch is a no-op (nothing is launched)


def test_write_predictions_lines_append_and_zip(tmp_path):
    from news_recommendation_model_amd import evaluation
    txt = str(tmp_path / "predictions.txt")
    n = evaluation.write_predictions(txt, [7, 12], [[3, 1, 2, 0], [1, 2, 0, 0]], [3, 2])
    assert n == 2 and open(txt, "rb").read() == b"7 [3,1,2]\n12 [1,2]\n"
    # numpy / torch inputs (float64 ids, as a DataLoader collates them), appended
    evaluation.write_predictions(txt, np.array([40.0]), torch.tensor([[2, 1, 3]], dtype=torch.int32), torch.tensor([3], dtype=torch.int32),
                                 append=True)
    assert open(txt, "rb").read() == b"7 [3,1,2]\n12 [1,2]\n40 [2,1,3]\n"
    evaluation.write_predictions(txt, [5], [[0, 0]], [0], append=True)    # no live candidate: an empty list
    assert open(txt, "rb").read().endswith(b"40 [2,1,3]\n5 []\n")
    with pytest.raises(ValueError):
        evaluation.write_predictions(txt, [1, 2], [[1, 2]], [2], append=True)
    with pytest.raises(ValueError):
        evaluation.write_predictions(txt, [1], [[1, 2]], [3], append=True)
    assert open(txt, "rb").read().count(b"\n") == 4                       # a refused call wrote nothing
    # the reference's own formatting of one row (test.py:124-130) gives the same bytes
    scores = [0.2, 0.5, 0.3]
    order = sorted(enumerate(scores), key=lambda x: x[1], reverse=True)
    want = ["-1"] * 3
    for r_i, (i, _v) in enumerate(order):
        want[i] = str(r_i + 1)
    assert evaluation.prediction_lines([9], [evaluation.rank_row(scores)], [3]) == "{} [{}]\n".format(9, ",".join(want))
    evaluation.write_predictions(txt, [1], [[1]], [1])                    # without append the file starts over
    assert open(txt, "rb").read() == b"1 [1]\n"
    zpath = evaluation.zip_predictions(txt, str(tmp_path / "predictions.zip"))
    with zipfile.ZipFile(zpath) as z:
        assert z.namelist() == ["predictions.txt"] and z.infolist()[0].compress_type == zipfile.ZIP_DEFLATED
        assert z.read("predictions.txt") == b"1 [1]\n"
    assert os.path.basename(zpath) == "predictions.zip"


def test_dataset_batches_stream_in_file_order(tmp_path):
    """score_dataset's reader: batches straddle subvolumes, keep file order, the last one is short."""
    from news_recommendation_model_amd import data_io, evaluation, synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(16, category_label_num=20)
    b = synth.make_batch(dims, 13, 3, 4, seed=2)
    b["impression_id"] = np.arange(100, 113)
    head = data_io.write_processed_dataset(data_io.records_from_batch(b), str(tmp_path / "test_set"), subvolume_item_num=6)
    got = list(evaluation.iter_dataset_batches(head, 5))
    assert [len(g["impression_id"]) for g in got] == [5, 5, 3]
    assert np.concatenate([g["impression_id"] for g in got]).tolist() == list(range(100, 113))
    assert np.array_equal(np.concatenate([g["x_target"] for g in got]), b["x_target"])


def test_ensemble_rank_op_is_registered_with_a_fake_and_refuses_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import ops
    assert "ensemble_rank" in ops.OPS and hasattr(torch.ops.nrm, "ensemble_rank")
    schema = str(torch.ops.nrm.ensemble_rank.default._schema)
    assert "Tensor[] logits" in schema and "Tensor? empty" in schema and "Tensor? label" in schema
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.ensemble_rank([torch.zeros(2, 3)], None, None)
    with FakeTensorMode():
        x = torch.empty(5, 7, device="cuda")
        for label, rows in ((None, 0), (torch.empty(5, 7, device="cuda"), 5)):
            score, rank, live, metrics = torch.ops.nrm.ensemble_rank([x, x], torch.empty(5, dtype=torch.int32, device="cuda"), label)
            assert (tuple(score.shape), score.dtype) == ((5, 7), torch.float32)
            assert (tuple(rank.shape), rank.dtype) == ((5, 7), torch.int32)
            assert (tuple(live.shape), live.dtype) == ((5,), torch.int32)
            assert (tuple(metrics.shape), metrics.dtype) == ((rows, 3), torch.float32)
