"""The device-side ScanQA / SQA3D batch on the GPU (csrc/gps_obj_select_qa.hip through sceneverse_amd/data/gpu_qa.py:
PackedQuestions, qa_rows): replays of the reference's shuffles and choices against the reference's own outputs
(tests/golden/qa_rows_ref.npz), bit for bit on every output; the rows the reference cannot run against the restatement
of tests/qa_rows_cases.py; the device law against its numpy emulation; `out=` buffers; one graph capture with the seed
word advanced on the device; and one composition qa_rows -> obj_processing_post + text_batch -> the native QA forward.
Every comparison of the selection is exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import qa_rows_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_qa import qa_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "qa_rows_ref.npz"))
HOT = ("tgt_object_id", "tgt_object_label", "answer_label")
KEYS = ("row_obj", "n_sel", "n_rem", "n_tgt", "sent_idx", "sqa_type", "obj_labels") + HOT
_CACHE = {}


def _packed():
    """All cases' scans as ONE PackedScans and all rows as ONE PackedQuestions, packed once for the module."""
    if "packed" not in _CACHE:
        _CACHE["packed"] = C.pack(device=DEV)
    return _CACHE["packed"]


def _case(name):
    return next(c for c in C.CASES if c["name"] == name)


def _setup(case):
    """-> (scans, questions, the rows' question numbers, the global id of each row's first position, the case's text ids,
    the keyword arguments that describe the case)."""
    packed, questions, where = _packed()
    q0, text_ids = where[case["name"]]
    B = len(case["rows"])
    pred = case["pc_type"] == "pred"
    sids = [C.scene_id(case, b) for b in range(B)]
    first = np.asarray([(packed.scan_proposals(s) if pred else packed.scan_objects(s)).start for s in sids], dtype=np.int64)
    kw = dict(O=case["O"], n_answers=case["A"], pc_type=case["pc_type"], matched=case["kind"] == "scanqa",
              long=case["kind"] == "sqa3d", train=case["kind"] == "sqa3d")
    keep = C.keep_of(case)
    if keep.ndim == 2:                           # per variant of the WHOLE question table: the other cases' rows keep nothing
        full = np.zeros((questions.n_variants, C.N_LABELS), bool)
        v0 = int(questions.var_first[q0].item())
        full[v0:v0 + len(keep)] = keep
        keep = full
    if not pred:
        kw["keep"] = torch.from_numpy(keep)
    else:
        kw["n_labels"] = C.N_LABELS
    return packed, questions, np.arange(q0, q0 + B), first, text_ids, kw


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, case, what):
    """Every output of a launch against the restatement's (or the fixture's) arrays: shapes, dtypes and values."""
    hot = np.int64 if case["kind"] == "sqa3d" else np.float32
    assert set(got) == set(KEYS), set(got) ^ set(KEYS)
    for k in KEYS:
        if k not in want:
            continue
        dt = hot if k in HOT else want[k].dtype
        assert got[k].dtype == dt and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k].astype(dt)), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1)))
        if k in HOT:
            assert set(np.unique(got[k]).tolist()) <= {0, 1}, (what, k)


def _garbage(case, B):
    """Static buffers holding values no launch writes."""
    O, A = case["O"], case["A"]
    hot = torch.int64 if case["kind"] == "sqa3d" else torch.float32
    shapes = {"row_obj": (B, O), "obj_labels": (B, O), "tgt_object_id": (B, O), "tgt_object_label": (B, C.N_LABELS), "answer_label": (B, A)}
    dtypes = {"row_obj": torch.int32, "n_sel": torch.int32, "n_rem": torch.int32, "n_tgt": torch.int32, "sent_idx": torch.int32,
              "sqa_type": torch.int64, "obj_labels": torch.int64}
    return {k: torch.full(shapes.get(k, (B,)), 7, dtype=dtypes.get(k, hot), device=DEV) for k in KEYS}


# ---- replays of the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_replay_equals_the_reference(case):
    name, M = case["name"], case["M"]
    packed, questions, q, first, text_ids, kw = _setup(case)
    B = len(q)
    g = {k: GOLD[f"{name}/{k}"] for k in ("row_obj", "n_sel", "n_rem", "sqa_type", "obj_labels") + HOT}
    ref = dict(g, row_obj=np.where(g["row_obj"] >= 0, g["row_obj"] + first[:, None], -1).astype(np.int32))
    order, pick = GOLD[f"{name}/order"], GOLD[f"{name}/pick"]
    want = C.restate_case(case, order=order, pick=pick, offsets=first, text_ids=text_ids)
    for dev in ("cpu", DEV):                                                    # described on the host / on the device
        args = dict(kw, order=torch.from_numpy(order).to(dev), pick=torch.from_numpy(pick).to(dev))
        got = _np(qa_rows(packed, questions, torch.from_numpy(q).to(dev), M, **args))
        _same(got, ref, case, "reference")                                      # the reference's own outputs, bit for bit
        _same(got, want, case, "restatement")                                   # ... and n_tgt, sent_idx
    out = _garbage(case, B)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    res = qa_rows(packed, questions, q, M, out=out, **args)
    assert all(res[k].data_ptr() == ptrs[k] for k in KEYS)
    _same(_np(out), want, case, "out buffers")                                  # every element written: nothing stale
    res = qa_rows(packed, questions, q[::-1].copy(), M, out=out, **dict(args, order=args["order"].flip(0), pick=args["pick"].flip(0)))
    _same(_np(out), {k: v[::-1] for k, v in want.items()}, case, "out buffers reused")
    if case["O"] == M + 1:
        assert qa_rows(packed, questions, q, M, **{k: v for k, v in args.items() if k != "O"})["row_obj"].shape == (B, M + 1)


def test_evaluation_mode_takes_the_first_variant():
    case = _case("sqa_gt_M5_lang")
    packed, questions, q, first, text_ids, kw = _setup(case)
    order = GOLD[f"{case['name']}/order"]
    got = _np(qa_rows(packed, questions, q, case["M"], **dict(kw, train=False, order=torch.from_numpy(order))))
    zero = np.zeros(len(q), np.int32)
    want = C.restate_case(case, order=order, pick=zero, offsets=first, text_ids=text_ids)
    for k in ("row_obj", "n_sel", "sent_idx", "obj_labels"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["sent_idx"], text_ids[C.var_first(case)[:-1]])


# ---- the device law -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_equals_its_emulation(case):
    """Fill (stream S + 3) and pick (stream S + 4) equal the numpy emulation bit for bit, `ref=False` rows included."""
    M = case["M"]
    packed, questions, q, first, text_ids, kw = _setup(case)
    q_d = torch.from_numpy(q).to(DEV)            # on the device: the odd cases' 1025 positions would be refused on the host
    fills, picks = [], []
    for seed in (0, 20240521, (1 << 63) + (7 << 32) + 5):
        got = _np(qa_rows(packed, questions, q_d, M, seed=seed, **kw))
        _same(got, C.restate_case(case, seed=seed, offsets=first, text_ids=text_ids), case, seed)
        fills.append(got["row_obj"])
        picks.append(got["sent_idx"])
    assert not np.array_equal(fills[0], fills[1]) and not np.array_equal(fills[1], fills[2])
    if case["kind"] == "sqa3d":
        assert not np.array_equal(picks[0], picks[1]) or not np.array_equal(picks[1], picks[2])
    seed_dev = torch.full((1,), (1 << 40) + 9, dtype=torch.int64, device=DEV)
    got = _np(qa_rows(packed, questions, q_d, M, seed=77, seed_dev=seed_dev, **kw))
    _same(got, C.restate_case(case, seed=77 + (1 << 40) + 9, offsets=first, text_ids=text_ids), case, "seed_dev")
    assert int(seed_dev.item()) == (1 << 40) + 9


# ---- what the reference cannot run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qa_gt_M5_odd", "qa_pred_M5_odd"])
def test_replay_of_the_rows_the_reference_cannot_run(name):
    """The four definitions of include/gps_hip.h and out-of-range ids; an order entry out of range writes -1."""
    case = _case(name)
    packed, questions, q, first, text_ids, kw = _setup(case)
    B, M = len(q), case["M"]
    order = np.stack([np.random.default_rng(b).permutation(12)[:M] for b in range(B)]).astype(np.int32)
    order[0, 0], order[1, 1] = -1, 10 ** 6
    got = _np(qa_rows(packed, questions, torch.from_numpy(q).to(DEV), M, order=torch.from_numpy(order), **kw))
    want = C.restate_case(case, order=order, offsets=first, text_ids=text_ids)
    _same(got, want, case, name)
    sizes = [len(r["scan"][1]) for r in case["rows"]]
    over = sizes.index(1025)                                                    # a scan over the cap: the empty row
    assert got["n_sel"][over] == 0 and (got["row_obj"][over] == -1).all() and got["sent_idx"][over] == -1
    assert not any(got[k][over].any() for k in HOT) and (got["obj_labels"][over] == -100).all()
    with pytest.raises(ValueError, match="> 1024"):                             # ... which a host q_idx refuses
        qa_rows(packed, questions, q[over:over + 1], M, **kw)
    if name == "qa_gt_M5_odd":
        assert got["n_tgt"].tolist()[:6] == [1, 1, 2, 2, 5, 5] and (got["n_sel"][:6] == [5, 5, 5, 5, 5, 5]).all()
        assert got["tgt_object_id"][4].tolist() == [1, 1, 1, 1, 1, 0]           # k = 7 > M: the first M targets, nothing else
        assert got["row_obj"][0, 1] == -1 and got["obj_labels"][0, 1] == -100   # the hole of a bad order entry
        assert got["answer_label"][9].sum() == 2                                # ids 64 and 0 of [64, 65, 70, 1000000, 0]
    else:
        assert got["n_tgt"].tolist() == [5, 5, 0, 2] and got["tgt_object_id"][:2, :5].all()


def test_empty_rows_from_a_question_or_a_target_out_of_range():
    case = _case("qa_gt_M5")
    packed, questions, q, first, text_ids, kw = _setup(case)
    M, nq = case["M"], questions.n_questions
    want = C.restate_case(case, seed=5, offsets=first, text_ids=text_ids)
    q_bad = q.copy()
    q_bad[[1, 4]] = (-1, nq)
    got = _np(qa_rows(packed, questions, torch.from_numpy(q_bad).to(DEV), M, seed=5, **kw))
    rows = np.asarray([b for b in range(len(q)) if b not in (1, 4)])
    for k in KEYS:
        assert np.array_equal(got[k][rows], want[k][rows].astype(got[k].dtype)), k
        fill = {"row_obj": -1, "obj_labels": -100, "sent_idx": -1}.get(k, 0)
        assert (got[k][[1, 4]] == fill).all(), k
    # a target one past its scan / before it, written into the resident table behind finalize()'s check
    b = next(b for b, r in enumerate(case["rows"]) if len(r["tgt"]) == 2)
    at = int(questions.tgt_first[q[b]].item())
    saved = questions.tgt_id.clone()
    try:
        for bad in (int(questions.ann_range[q[b], 1].item()), int(questions.ann_range[q[b], 0].item()) - 1, -5, 2 ** 31 - 1):
            questions.tgt_id[at + 1] = bad
            got = _np(qa_rows(packed, questions, q, M, seed=5, **kw))
            assert got["n_sel"][b] == 0 and (got["row_obj"][b] == -1).all() and not any(got[k][b].any() for k in HOT), bad
            rows = np.asarray([i for i in range(len(q)) if i != b])
            assert all(np.array_equal(got[k][rows], want[k][rows].astype(got[k].dtype)) for k in KEYS), bad
    finally:
        questions.tgt_id.copy_(saved)
    assert qa_rows(packed, questions, [], M, **kw)["answer_label"].shape == (0, case["A"])


def test_wrapper_refusals_on_the_device():
    case = _case("qa_gt_M5")
    packed, questions, q, first, text_ids, kw = _setup(case)
    B, M = len(q), case["M"]
    good = _garbage(case, B)
    qa_rows(packed, questions, q, M, out=good, **kw)
    for bad in (dict(good, row_obj=good["row_obj"].long()), dict(good, answer_label=good["answer_label"].long()),
                dict(good, tgt_object_id=good["tgt_object_id"][:, :5]), {k: v for k, v in good.items() if k != "n_tgt"},
                dict(good, sqa_type=good["sqa_type"].cpu())):
        with pytest.raises(ValueError, match="out"):
            qa_rows(packed, questions, q, M, out=bad, **kw)
    for seed_dev in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="seed_dev"):
            qa_rows(packed, questions, q, M, seed_dev=seed_dev, **kw)
    with pytest.raises(ValueError, match="question number outside"):
        qa_rows(packed, questions, [questions.n_questions], M, **kw)


# ---- one capture, fresh fill and pick per replay -----------------------------------------------------------------------------
def test_graph_replays_draw_fresh_fills_and_picks():
    """Advance the seed word on the device, build the batch, build the object tensors from its rows: three replays, each
    equal to the emulation at the advanced seed, the fills and the picks different between them."""
    case = _case("sqa_gt_M5")
    packed, questions, q, first, text_ids, kw = _setup(case)
    M = case["M"]
    q_d = torch.from_numpy(q).to(device=DEV, dtype=torch.int32)
    seed, start = 1000, 41
    seed_dev = torch.full((1,), start, dtype=torch.int64, device=DEV)
    kw = dict(kw, keep=kw["keep"].to(DEV), seed=seed, seed_dev=seed_dev)
    out = qa_rows(packed, questions, q_d, M, **kw)            # the buffers, and the library loaded ahead of the capture
    post = G.obj_processing_post(packed, out["row_obj"], num_points=8)
    _same(_np(out), C.restate_case(case, seed=seed + start, offsets=first, text_ids=text_ids), case, "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seed_dev.add_(1)
        qa_rows(packed, questions, q_d, M, out=out, **kw)
        G.obj_processing_post(packed, out["row_obj"], num_points=8, out=post)
    fills, picks = [], []
    for k in range(1, 4):
        graph.replay()
        got = _np(out)
        want = C.restate_case(case, seed=seed + start + k, offsets=first, text_ids=text_ids)
        _same(got, want, case, k)
        assert np.array_equal(post["obj_masks"].cpu().numpy(), want["row_obj"] >= 0)
        fills.append(got["row_obj"])
        picks.append(got["sent_idx"])
    assert int(seed_dev.item()) == start + 3
    pairs = ((0, 1), (0, 2), (1, 2))
    assert not any(np.array_equal(fills[a], fills[b]) for a, b in pairs)
    assert not any(np.array_equal(picks[a], picks[b]) for a, b in pairs)


# ---- the composition: a QA data_dict from one question id per row -----------------------------------------------------------
def test_a_qa_batch_from_one_question_id_per_row_runs_the_native_forward():
    from oracle.param_fill import fill_params
    from sceneverse_amd.data.gpu_text import text_batch
    from sceneverse_amd.data.synthetic import synth_packed_questions, synth_packed_texts, synth_qa_batch
    from sceneverse_amd.model.build import build_model
    from sceneverse_amd.optim.loss.loss import answer_loss
    from tests.qa_cases import as_qa_cfg
    from tests.util import gps_cfg, lang_dir
    B, M, O, P, L, A = 2, 5, 6, 1024, 12, 8864
    case = _case("qa_pred_M5")                                                  # its scans' 13 ANNOTATED cubes, 12 of them foreground
    packed, _, _, _, _, _ = _setup(case)
    sids = [C.scene_id(case, b) for b in (8, 9, 10)]
    texts = synth_packed_texts(12, 2, seed=5, device=DEV, txt_len=L, scene_txt_len=8)
    questions = synth_packed_questions(packed, sids, 6, n_texts=12, seed=9, n_answers=A)
    keep = G.keep_table(C.INT2CAT)
    rows = qa_rows(packed, questions, [4, 1], M, O=O, n_answers=A, keep=keep, long=True, seed=3)
    post = G.obj_processing_post(packed, rows["row_obj"], num_points=P, need_boxes=True)
    buf = {k: torch.full((B, 8 if k.startswith("scene") else L), 7, dtype=torch.int64, device=DEV)
           for k in ("txt_ids", "txt_masks", "masked_lm_labels", "scene_txt_ids", "scene_txt_masks")}
    buf["obj_sem_masks"] = torch.ones((B, O), dtype=torch.bool, device=DEV)
    txt = text_batch(texts, rows["sent_idx"], torch.tensor([12, 13]), max_seq_len=L, max_scene_cap_len=8, mask=False,
                     obj_masks=post["obj_masks"], out=buf)
    data = {**{k: post[k] for k in ("obj_fts", "obj_locs", "obj_masks")}, **txt,
            **{k: rows[k] for k in ("obj_labels", "tgt_object_id", "answer_label", "sqa_type")}}
    assert bool((data["masked_lm_labels"] == -1).all())                        # mask=False: no label anywhere
    ref = synth_qa_batch(B, n_obj=O, n_pts=P, txt_len=L, n_answers=A, seed=1)
    assert set(data) == set(ref)
    for k, v in ref.items():
        assert data[k].shape == v.shape and data[k].dtype == v.dtype, (k, data[k].shape, data[k].dtype, v.shape, v.dtype)
    assert torch.equal(post["obj_masks"].sum(1).int(), rows["n_sel"]) and bool((rows["n_sel"] == M).all())
    assert torch.equal(data["obj_sem_masks"], data["obj_masks"])
    cfg = as_qa_cfg(gps_cfg(lang_dir(11), heads="pretrain", use_scene_cap=False))
    model = build_model(cfg).eval()
    fill_params(model, 11)
    model.to(DEV)
    with torch.no_grad():
        out = model(data)
        loss = answer_loss({"answer_scores": out["answer_scores"], "answer_label": data["answer_label"]})
    assert out["answer_scores"].shape == (B, A) and bool(torch.isfinite(out["answer_scores"]).all())
    assert bool(torch.isfinite(loss))
