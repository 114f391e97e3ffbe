"""The launch sequence behind tests/golden/launch_table_parent.json, shared by tests/golden/make_golden_launch_table.py
(which recorded it at the commit before the native launch got one definition) and tests/test_gpu_launch_table.py (which
reruns it).  It reads the launch profiler through `_ext.profile_start()` / `_ext.profile_stop()` only.

What runs, each at the smallest case the suite already uses:
  one eager pre-train step (bench.gps_pretrain_cfg, 2 scenes x 8 objects, HIP graph off, seeds fixed);
  the QA head + answer_loss              tests/qa_cases.py      "sqa3d", fp32, backend 'hip';
  the grounding head + native og3d loss  tests/ground_cases.py  "plain", fp32, backend 'hip';
  the ScanRefer targets                  tests/refer_cases.py   "pred8";
  the metrics fold                       tests/metrics_cases.py "pre_min", batch 0, PretrainCounter update + result.
Per profile key the table holds the launch count, the algorithmic FLOPs and bytes per launch (integer expressions of the
shapes and of seeded extent words), the MFMA dtype and whether a work fraction was recorded.  Nothing timed is kept."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIELDS = ("launches", "flops_per_launch", "bytes_per_launch", "mfma_dtype")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_table_parent.json")


def _sequence(dev):
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.data import gpu_objects as G
    from sceneverse_amd.data.synthetic import synth_batch
    from sceneverse_amd.engine import GPSTrainStep, PretrainCounter
    from sceneverse_amd.modules.heads import grounding_head, qa_head
    from sceneverse_amd.optim.loss import loss as L
    from tests import ground_cases, metrics_cases, qa_cases, refer_cases

    torch.manual_seed(0)
    step = GPSTrainStep(gps_pretrain_cfg(_lang_dir()), device=dev, ddp=False, graph=False, seed=7)
    step.step(synth_batch(2, n_obj=8, seed=0, min_real=3, device=dev))

    qa_head.set_qa_backend("hip")
    try:
        qa_cases.run_head(dev, qa_cases.load_gold(), "sqa3d", 2e-3, qa_cases.FP32_GPU_GRADS)
    finally:
        qa_head.set_qa_backend("auto")

    grounding_head.set_ground_backend("hip")
    fused, L._FUSED_OG3D = L._FUSED_OG3D, True
    try:
        ground_cases.run_head(dev, ground_cases.load_gold(), "plain", 2e-3, ground_cases.FP32_GPU_GRADS)
    finally:
        grounding_head.set_ground_backend("auto")
        L._FUSED_OG3D = fused

    packed = refer_cases.pack(device=dev)
    case = refer_cases.CASES[0]
    rows, tgt, sids = refer_cases.case_inputs(packed, case)
    G.refer_targets(packed, rows, tgt, sids, case[2])

    counter = PretrainCounter(dev)
    counter.update(metrics_cases.to_device(metrics_cases.batch("pre_min", 0), dev))
    counter.result()


def launch_table(dev="cuda"):
    """-> {profile key: {launches, flops_per_launch, bytes_per_launch, mfma_dtype, work_fraction: bool}}"""
    from sceneverse_amd.pointnet2 import _ext
    _ext.profile_start()
    try:
        _sequence(dev)
    finally:
        rec = _ext.profile_stop()
    return {k: dict({f: v[f] for f in FIELDS}, work_fraction="work_fraction" in v) for k, v in sorted(rec.items())}
