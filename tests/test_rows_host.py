"""The device-side object selection on the host: the numpy restatement of tests/rows_cases.py against the reference's own
outputs (tests/golden/rows_ref.npz, written by tests/golden/make_golden_rows.py) -- exact; the statistics of the device
fill law on its numpy emulation; the argument checks of gps_obj_select, which come before any launch; and the wrapper's
host-side refusals.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rows_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_objects import keep_table, select_rows  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "rows_ref.npz"))


def test_entry_is_declared_bound_and_built():
    lib = _native.load()
    assert "gps_obj_select" in _native.declared_symbols() and "gps_obj_select" in _native.SIGNATURES
    assert hasattr(lib, "gps_obj_select") and lib.gps_abi_version() == 11       # additive: the ABI number does not move
    from sceneverse_amd.csrc import build
    assert ("gps_obj_select.hip", []) in build.SOURCES
    text = open(_native.HEADER_PATH).read()
    for cite in ("base.py:231-246", "base.py:275-289", "base.py:368-450", "base.py:877-957", "scannet.py:70-76",
                 "#define GPS_OBJ_SELECT_MAX_SCAN 1024"):
        assert cite in text, cite
    assert G.OBJ_SELECT_MAX_SCAN == C.MAX_SCAN == 1024


@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_restatement_equals_the_reference(case):
    name = case["name"]
    got = C.restate_case(case, order=GOLD[f"{name}/order"])
    assert np.array_equal(got["row_obj"], GOLD[f"{name}/sel"])
    for k in ("tgt_slot", "n_sel", "n_rem", "is_multiple", "is_hard"):
        assert np.array_equal(got[k], GOLD[f"{name}/{k}"]), k
    assert GOLD[f"{name}/order"].shape == (len(case["scans"]), case["M"])


def test_fixture_covers_the_cases_it_claims():
    for M in C.MS:
        case = next(c for c in C.CASES if c["name"] == f"refer_M{M}")
        g = {k: GOLD[f"refer_M{M}/{k}"] for k in ("sel", "tgt_slot", "n_sel", "n_rem", "order")}
        lens = [len(s) for s in case["scans"]]
        assert lens[:6] == [1, 63, 64, 65, 130, 1024]
        keep = C.keep_fg()
        n = np.asarray([int(keep[s].sum()) + (0 if keep[s[t]] else 1) for s, t in zip(case["scans"], case["tgt"])])
        assert (n == M).any() and (n == M + 1).any() and (n < M).any()
        cropped = n > M
        assert (g["tgt_slot"][cropped] == 0).all() and (g["n_sel"][cropped] == M).all()
        assert np.array_equal(g["n_sel"][~cropped], n[~cropped])
        fill = g["n_rem"] > 0
        free = np.asarray([M - 1 - sum(1 for p in range(len(s)) if p != t and keep[s[p]] and s[p] == s[t])
                           for s, t in zip(case["scans"], case["tgt"])])
        assert (fill == (cropped & (free > 0))).all()
        assert ((g["n_rem"] - free)[fill] == 1).any()                      # all but one of remained
        assert (free[cropped] == 1).any() and (free[cropped] == 0).any() and (free[cropped] < 0).any()   # M-2, M-1, M mates
        assert any(t == 0 for t in case["tgt"]) and any(t == len(s) - 1 for s, t in zip(case["scans"], case["tgt"]))
        walls = [b for b, (s, t) in enumerate(zip(case["scans"], case["tgt"])) if s[t] == 0 and len(s) > 1]
        assert any(g["tgt_slot"][b] == M - 1 and n[b] == M for b in walls)  # appended last, no crop
        assert any(g["tgt_slot"][b] == 0 and n[b] == M + 1 for b in walls)
        assert any(t > 64 for t in case["tgt"])
        # a replay order is a permutation prefix of range(n_rem)
        for b in np.flatnonzero(fill):
            o = g["order"][b][:min(M, g["n_rem"][b])]
            assert len(set(o.tolist())) == len(o) and o.min() >= 0 and o.max() < g["n_rem"][b]
    # the map merges two labels: is_multiple differs from the identity's somewhere, is_hard never
    case = next(c for c in C.CASES if c["name"] == "refer_M79_map")
    plain = C.restate_case(dict(case, label_map=None), order=GOLD["refer_M79_map/order"])
    assert not np.array_equal(plain["is_multiple"], GOLD["refer_M79_map/is_multiple"])
    assert np.array_equal(plain["is_hard"], GOLD["refer_M79_map/is_hard"])
    # the per-row table and the CLASS_LABELS_200 filter select differently from the plain one
    for name in ("refer_M5_lang", "objpretrain_M5"):
        case = next(c for c in C.CASES if c["name"] == name)
        plain = C.restate_case(dict(case, keep="fg"), order=GOLD[f"{name}/order"])
        assert not np.array_equal(plain["row_obj"], GOLD[f"{name}/sel"])
    assert C.keep_of(next(c for c in C.CASES if c["name"] == "refer_M5_lang")).ndim == 2


def test_keep_table():
    assert np.array_equal(keep_table(C.INT2CAT).numpy(), C.keep_fg())
    assert np.array_equal(keep_table(C.INT2CAT, only=C.IN_200).numpy(), C.keep_200())
    assert keep_table(C.INT2CAT, drop=()).all() and keep_table(C.INT2CAT).dtype == torch.bool
    assert keep_table(C.INT2CAT, only=("chair", "wall")).tolist() == [c == "chair" for c in C.INT2CAT]


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_gives_a_permutation_of_remained(case):
    seed = (5 << 60) + 17
    got = C.restate_case(case, seed=seed)
    keep = C.keep_of(case)
    for b, (labels, t) in enumerate(zip(case["scans"], case["tgt"])):
        n_rem = int(got["n_rem"][b])
        o = C.device_order(seed, b, n_rem)
        assert sorted(o.tolist()) == list(range(n_rem))
        row = got["row_obj"][b][:got["n_sel"][b]]
        assert len(set(row.tolist())) == len(row) and (row >= 0).all() and (row < len(labels)).all()
        k = keep if keep.ndim == 1 else keep[b]
        ok = [0 <= labels[p] < C.N_LABELS and k[labels[p]] for p in row]
        assert all(ok[i] or (case["mode"] == "refer" and row[i] == t) for i in range(len(row)))
        assert (got["row_obj"][b][got["n_sel"][b]:] == -1).all()
        if n_rem:                                                              # the fill is a prefix of the shuffled remained
            assert got["n_sel"][b] == case["M"]
    # the same seed gives the same rows, another seed another fill
    again, other = C.restate_case(case, seed=seed), C.restate_case(case, seed=seed + 1)
    assert np.array_equal(again["row_obj"], got["row_obj"])
    if (got["n_rem"] > 0).any():
        assert not np.array_equal(other["row_obj"], got["row_obj"])
    assert np.array_equal(other["n_rem"], got["n_rem"]) and np.array_equal(other["is_hard"], got["is_hard"])


# ---- the device law on its emulation ----------------------------------------------------------------------------------
N_ROWS = 65536
SEEDS = (0, 20240521, (1 << 63) + (7 << 32) + 5)


def _z(count, p, n):
    return abs(count - n * p) / math.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", [(10, 4), (80, 30)], ids=["10of4", "80of30"])
def test_device_law_statistics(shape, seed):
    """Every object of remained is included in k / n_rem of the rows and comes first in 1 / n_rem of them: each count
    within 5 binomial standard deviations (a fair shuffle leaves that band with probability 5.7e-7 per count; an
    emulation of the same law on the neighbouring stream stayed within 3.6)."""
    n_rem, k = shape
    ranks = C.fill_ranks(seed, N_ROWS, n_rem)
    assert (np.sort(ranks, axis=1) == np.arange(n_rem)[None, :]).all()
    included, first = (ranks < k).sum(0), (ranks == 0).sum(0)
    z_in = max(_z(int(c), k / n_rem, N_ROWS) for c in included)
    z_first = max(_z(int(c), 1.0 / n_rem, N_ROWS) for c in first)
    print(f"seed {seed}: (n_rem, k) = {shape}: worst z inclusion {z_in:.2f}, first place {z_first:.2f}")
    assert z_in <= 5.0 and z_first <= 5.0
    # one row of fill_ranks is device_order's inverse
    assert np.array_equal(np.argsort(ranks[3]), C.device_order(seed, 3, n_rem))


def test_device_law_uses_its_own_stream():
    from text_cases import rng_u32
    r = np.arange(16, dtype=np.uint64)
    h = rng_u32(7 + 3, np.uint64(2) * np.uint64(1 << 20) + r)
    assert np.array_equal(C.device_order(7, 2, 16), np.argsort((h << np.uint64(32)) | r))
    assert not np.array_equal(C.device_order(7, 2, 16), C.device_order(7, 3, 16))
    assert np.array_equal(C.device_order((1 << 64) - 3, 0, 16), np.argsort(rng_u32(0, r), kind="stable"))     # S + 3 wraps


# ---- the C entry's checks -----------------------------------------------------------------------------------------------
def _call(lib, **kw):
    """gps_obj_select with a valid argument set (non-NULL stand-in addresses: nothing is launched when a check fails
    first) in which the named arguments are replaced."""
    a = dict(B=2, O=80, M=79, mode=0, n_objects=100, n_labels=12, labels=16, scan_range=16, tgt_obj=16, keep=16,
             keep_stride=0, label_map=None, order=None, R=0, seed=0, seed_dev=None, row_obj=16, tgt_slot=16, n_sel=16,
             n_rem=16, is_multiple=16, is_hard=16, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return lib.gps_obj_select(*a.values())


def test_argument_checks_come_before_any_launch():
    lib = _native.load()
    OK, INVALID, UNSUPPORTED = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT, _native.GPS_ERR_UNSUPPORTED
    for bad in (dict(B=-1), dict(O=-1), dict(n_objects=-1), dict(n_labels=-1), dict(R=-1), dict(M=0), dict(M=-3),
                dict(M=81), dict(mode=2), dict(mode=-1), dict(keep_stride=1), dict(keep_stride=-12), dict(order=16, R=78),
                dict(order=16, R=0), dict(labels=None), dict(scan_range=None), dict(tgt_obj=None), dict(keep=None),
                dict(row_obj=None), dict(tgt_slot=None), dict(n_sel=None), dict(n_rem=None), dict(is_multiple=None),
                dict(is_hard=None)):
        assert _call(lib, **bad) == INVALID, bad
    assert _call(lib, M=1, O=1) == UNSUPPORTED and _call(lib, M=1, O=2) == UNSUPPORTED       # refer mode needs M >= 2
    assert _call(lib, O=513) == UNSUPPORTED and _call(lib, O=513, M=513) == UNSUPPORTED
    none = dict(labels=None, scan_range=None, tgt_obj=None, keep=None, row_obj=None, tgt_slot=None, n_sel=None,
                n_rem=None, is_multiple=None, is_hard=None)
    assert _call(lib, B=0, **none) == OK and _call(lib, B=0, mode=1, M=1, O=1, **none) == OK
    assert _call(lib, B=0, M=0, **none) == INVALID and _call(lib, B=0, M=1, **none) == UNSUPPORTED
    assert _call(lib, B=0, keep_stride=5, **none) == INVALID


# ---- the wrapper's refusals, all raised before a device is touched --------------------------------------------------------
def _packed(sizes):
    p = G.PackedScans("cpu")
    for i, n in enumerate(sizes):
        p.add_scan(f"s{i}", np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8), np.arange(n), list(range(n)),
                   inst_labels=[3] * n)
    return p.finalize()


def test_wrapper_refusals():
    packed = _packed([4, 1025])
    keep = keep_table(C.INT2CAT)
    with pytest.raises(ValueError, match="1025 objects > 1024"):
        select_rows(packed, ["s0", "s1"], 5, tgt_obj=[0, 0], keep=keep)
    with pytest.raises(ValueError, match="max_keep"):
        select_rows(packed, ["s0"], 5, O=4, tgt_obj=[0], keep=keep)
    with pytest.raises(ValueError, match="max_keep"):
        select_rows(packed, ["s0"], 0, mode="pretrain", keep=keep)
    with pytest.raises(ValueError, match="max_keep >= 2"):
        select_rows(packed, ["s0"], 1, tgt_obj=[0], keep=keep)
    with pytest.raises(ValueError, match="tgt_obj"):
        select_rows(packed, ["s0"], 5, keep=keep)
    with pytest.raises(ValueError, match="outside its scan"):
        select_rows(packed, ["s0"], 5, tgt_obj=[4], keep=keep)
    with pytest.raises(ValueError, match="object slots"):
        select_rows(packed, ["s0"], 5, O=513, tgt_obj=[0], keep=keep)
    with pytest.raises(ValueError, match="mode"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], keep=keep, mode="pred")
    with pytest.raises(ValueError, match="keep"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], keep=keep)
    with pytest.raises(RuntimeError, match="finalize"):
        select_rows(G.PackedScans("cpu"), [], 5, tgt_obj=[], keep=keep)
    # batch_rows is as it was: it copies ranges and refuses the scan select_rows exists for
    with pytest.raises(ValueError, match="> max_obj_len"):
        G.batch_rows(packed, ["s1"], 80)
    assert G.batch_rows(packed, ["s0"], 6).tolist() == [[0, 1, 2, 3, -1, -1]]
    assert G.scan_ranges(packed, ["s1", "s0"]).tolist() == [[4, 1029], [0, 4]]
