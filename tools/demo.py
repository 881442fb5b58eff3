"""The reference's scripts/demo.py on the engine: infer() on tests/golden/demo/rgb.png with its intrinsics, the ARel against depth.png, and
the artifact rgb | gt / pred | error rendered on the GPU by demo_panel (one ud_colorize call) and written by save_png.

    python tools/demo.py [--out demo_output.png] [--arch vitl14] [--checkpoint DIR]

Weights: --checkpoint, else $UNIDEPTH_V2_VITL14_DIR or the local Hugging Face cache of lpiccinelli/unidepth-v2-vitl14 (nothing is
downloaded); when none is present, a seeded synthetic checkpoint as bench.py makes one -- the picture then shows the plumbing, not a
depth estimate, and the printed ARel means nothing.  Reading the two PNGs uses PIL."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
REPO_ID = "lpiccinelli/unidepth-v2-vitl14"


def released_checkpoint_dir():
    d = os.environ.get("UNIDEPTH_V2_VITL14_DIR", "")
    if d and os.path.isfile(os.path.join(d, "config.json")):
        return d
    try:
        from huggingface_hub import snapshot_download
        d = snapshot_download(REPO_ID, allow_patterns=["config.json", "model.safetensors", "pytorch_model.bin"], local_files_only=True)
    except Exception:
        return None
    return d if any(os.path.isfile(os.path.join(d, f)) for f in ("model.safetensors", "pytorch_model.bin")) else None


def load_model(arch, checkpoint):
    from unidepth_amd import UniDepthV2
    ckpt = checkpoint or released_checkpoint_dir()
    if ckpt:
        print("weights:", ckpt)
        model = UniDepthV2.from_pretrained(ckpt)
    else:
        from oracle import synth
        print(f"weights: none found, seeded synthetic {arch} checkpoint (the output is not a depth estimate)")
        cfg = synth.load_config(arch)
        model = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, 125))
    return model.to("cuda").eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="demo_output.png")
    ap.add_argument("--arch", default="vitl14", help="architecture of the synthetic checkpoint when no released weights are found")
    ap.add_argument("--checkpoint", default="", help="directory with config.json and the released weights")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/demo.py needs the GPU"
    from PIL import Image
    from unidepth_amd import demo_panel, save_png
    from unidepth_amd.cameras import Pinhole

    with Image.open(os.path.join(DEMO, "rgb.png")) as im:
        rgb = torch.from_numpy(np.asarray(im, dtype=np.uint8).transpose(2, 0, 1).copy())         # u8 [3, H, W]
    with Image.open(os.path.join(DEMO, "depth.png")) as im:
        gt_m = np.asarray(im, dtype=np.float64) * 1e-3                                          # uint16 millimetres -> metres; 0 = no truth
    K = torch.from_numpy(np.load(os.path.join(DEMO, "intrinsics.npy")))

    model = load_model(args.arch, args.checkpoint)
    out = model.infer(rgb, Pinhole(K=K[None]))
    gt = torch.from_numpy(gt_m.astype(np.float32)).cuda()
    artifact = demo_panel(rgb.cuda(), out["depth"], gt[None])                  # depth 0.01..10 magma_r, error 0..0.2 coolwarm
    save_png(args.out, artifact[0])

    pred_m = out["depth"].reshape(gt_m.shape).double().cpu().numpy()
    known = gt_m > 0
    arel = float((np.abs(gt_m[known] - pred_m[known]) / gt_m[known]).mean())
    print("Available predictions:", sorted(out))
    print("ARel: %.2f%%" % (100.0 * arel))
    print("wrote", args.out, tuple(artifact.shape[1:]))


if __name__ == "__main__":
    main()
