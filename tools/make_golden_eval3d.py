"""Writes tests/golden/eval_3d_batch.npz: the REFERENCE's eval_3d (unidepth/utils/evaluation_depth.py:160-182 over its chamfer class
and its own CPU K-NN extension compiled from its sources, oracle/make_golden_eval.reference_knn_module / reference_eval_3d) run on
the CPU on the seeded inputs of tests/eval3d_restate.case_inputs.  Only the reference's outputs are stored, a few floats per case;
needs the reference checkout of the authoring container.

    python tools/make_golden_eval3d.py"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval3d_restate as er  # noqa: E402
from oracle import make_golden_eval  # noqa: E402


def main():
    ev3d = make_golden_eval.reference_eval_3d(make_golden_eval.reference_knn_module())
    out = {}
    for name in er.CASES:
        gts, preds, masks, th = er.case_inputs(name)
        t0 = time.time()
        with torch.no_grad():
            res = ev3d(gts, preds, masks, th)
        for k in er.KEYS:
            out[f"{name}.{k}"] = res[k].numpy().astype(np.float32)
        print(f"{name}: {len(res['F1'])} rows in {time.time() - t0:.1f} s", {k: out[f'{name}.{k}'] for k in er.KEYS}, flush=True)
    np.savez_compressed(er.GOLDEN, **out)
    print("wrote", er.GOLDEN)


if __name__ == "__main__":
    main()
