"""data/_resident.py: the `out=` contract of every resident-batch call, checked on plain CPU tensors (tensor metadata only)."""
import pytest
import torch

from sceneverse_amd.data import _resident as R

CPU = torch.device("cpu")
SPEC = (("rows", torch.int32, (2, 3)), ("flag", torch.bool, (2,)), ("mask", torch.uint8, (2, 3)))


def _good():
    return {"rows": torch.zeros((2, 3), dtype=torch.int32), "flag": torch.zeros(2, dtype=torch.bool),
            "mask": torch.zeros((2, 3), dtype=torch.uint8)}


def test_outputs_allocates_the_spec():
    res = R.outputs("f", SPEC, None, CPU, "scans")
    assert list(res) == ["rows", "flag", "mask"]
    for name, dt, shape in SPEC:                                               # a flag is allocated as the spec names it
        assert res[name].dtype == dt and tuple(res[name].shape) == shape and res[name].device == CPU


def test_outputs_hands_back_the_callers_tensors():
    out = dict(_good(), extra=torch.zeros(1))
    res = R.outputs("f", SPEC, out, CPU, "scans")
    assert list(res) == ["rows", "flag", "mask"] and all(res[k] is out[k] for k in res)


@pytest.mark.parametrize("name,bad", [
    ("rows", torch.zeros((2, 4), dtype=torch.int32)),                          # shape
    ("rows", torch.zeros((2, 3), dtype=torch.int64)),                          # dtype
    ("flag", torch.zeros(2, dtype=torch.int32)),                               # a flag is one byte
    ("rows", torch.zeros((3, 2), dtype=torch.int32).t()),                      # not contiguous
    ("mask", torch.zeros((2, 6), dtype=torch.uint8)[:, ::2]),
    ("rows", torch.zeros((2, 3), dtype=torch.int32, device="meta")),           # another device
    ("flag", None),                                                            # missing: the same error
])
def test_outputs_refuses_by_name(name, bad):
    out = _good()
    if bad is None:
        del out[name]
    else:
        out[name] = bad
    with pytest.raises(ValueError) as e:
        R.outputs("select_rows", SPEC, out, CPU, "scans")
    want = {n: (dt, shape) for n, dt, shape in SPEC}[name]
    assert str(e.value) == f"select_rows: out[{name!r}] must be a contiguous {want[1]} {want[0]} tensor on the scans' GPU"


def test_flags_as_bool():
    out = dict(_good(), flag=torch.tensor([1, 0], dtype=torch.uint8), mask=torch.zeros((2, 3), dtype=torch.bool))
    res = R.outputs("f", SPEC, out, CPU, "scans")                              # uint8 for bool and bool for uint8
    flag, mask = res["flag"], res["mask"]
    assert R.as_bool(res, ("flag", "mask", "absent")) is res
    assert res["mask"] is mask                                                 # already bool: the caller's own object
    assert res["flag"].dtype == torch.bool and res["flag"].tolist() == [True, False]
    assert res["flag"].data_ptr() == flag.data_ptr()                           # a view: written in place, seen through it
    flag[1] = 1
    assert res["flag"].tolist() == [True, True]
    assert res["rows"].dtype == torch.int32


def test_guards_and_seed_word():
    with pytest.raises(RuntimeError, match=r"PackedScans.finalize\(\) has not been called"):
        R.need_finalized(None, "PackedScans")
    R.need_finalized(torch.zeros(1), "PackedScans")
    with pytest.raises(RuntimeError, match=r"select_rows runs on libgps_hip.so: scenes must live on a GPU \(no CPU path\)"):
        R.need_gpu(CPU, "select_rows", "scenes")
    R.seed_word("f", None, CPU, "texts")
    R.seed_word("f", torch.zeros(1, dtype=torch.int64), CPU, "texts")
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                torch.zeros(1, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="f: seed_dev must be one int64 word on the texts' GPU"):
            R.seed_word("f", bad, CPU, "texts")
    assert R.u64(-1) == (1 << 64) - 1 and R.u64(1 << 64) == 0 and R.u64(7) == 7
