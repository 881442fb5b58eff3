"""ud_eval_depth (csrc/evaldepth.hip) at its edges, against the numpy restatement of tools/make_golden_eval_depth.py (pinned to the
reference's golden file by tests/test_eval_depth_cpu.py) under that module's compare(): pixel counts on both sides of the 4096-pixel
chunk with images that are full, nearly empty and valid in the last chunk only; ratios exactly on every counting threshold, where the
counts are known from the construction and must be reproduced to the bit; depths whose radix digits all differ; the C-ABI with a
guarded output, a padded and dirty work area and mask = NULL under max_depth; and the wrapper's layouts, fp16 and graph capture."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import layout_guard as lg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_eval_depth", os.path.join(ROOT, "tools", "make_golden_eval_depth.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

ED_CHUNK = 4096                            # pixels per block of every pass (csrc/evaldepth.hip)


def _run(gts, preds, masks, max_depth=None):
    from unidepth_amd import eval_ops
    res = eval_ops.eval_depth(gts.cuda(), preds.cuda(), masks.cuda(), max_depth=max_depth)
    assert tuple(res) == mg.KEYS
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in mg.KEYS)


def _cabi(gt, pred, mask, max_depth, work_fill=0x00, calls=1):
    """ud_eval_depth driven directly on contiguous fp32 gt [B,H,W], pred [B,h,w], u8 mask [B,H,W] or None: out a guarded row of 18 * B
    floats, work inside 0xA5 padding and pre-filled with `work_fill`; `calls` launches into the same buffers.  -> {key: [B]} numpy."""
    from unidepth_amd import _lib, eval_ops
    from unidepth_amd.ops import cur_stream, mk
    B, H, W = gt.shape
    h, w = pred.shape[1:]
    nbytes = int(_lib.lib.ud_eval_depth_work_bytes(B, H, W))
    assert nbytes > 0
    wpad = 4096
    wbuf = torch.full((wpad + nbytes + wpad,), 0xA5, dtype=torch.uint8, device="cuda")
    wbuf[wpad:wpad + nbytes] = work_fill
    og = lg.guarded(1, 18 * B, 18 * B + 7, torch.float32, pre_rows=2, post_rows=2, offset_cols=3)
    d = mk(_lib.UdEvalDepth, gt=gt, pred=pred, mask=mask, thresholds=eval_ops._dauc_thresholds(gt.device), out=og.ptr(),
           work=wbuf[wpad:wpad + nbytes], B=B, H=H, W=W, h=h, w=w, max_depth=0.0 if max_depth is None else float(max_depth),
           has_max_depth=0 if max_depth is None else 1, work_bytes=nbytes)
    for _ in range(calls):
        _lib.check(_lib.lib.ud_eval_depth(C.byref(d), cur_stream()), "ud_eval_depth")
    torch.cuda.synchronize()
    og.check_guards("out")
    assert bool((wbuf[:wpad] == 0xA5).all()) and bool((wbuf[wpad + nbytes:] == 0xA5).all()), "work area: guard rewritten"
    rows = og.view.reshape(18, B).cpu().numpy()
    return {k: rows[i].copy() for i, k in enumerate(mg.KEYS)}


# ---- pixel counts around the chunk ----------------------------------------------------------------------------------------------------

def _chunk_inputs(HW, resampled):
    """B = 3 images of 1 x HW: all valid; the first and the last pixel only; the pixels of the last chunk only.

    The two pixels of image 1 get log-ratios d = ln p - ln g of +ln 1.3 and -ln 1.2.  With n = 2, silog = 100 |d0 - d1| / sqrt(2), and
    every d is the difference of two fp32 logarithms (|ln| < 2.5, one unit in the last place 2.4e-7), so it carries about 5e-7 of
    rounding in the kernel and in the numpy restatement alike; compare()'s relative 1e-5 can only be asked of either when
    |d0 - d1| > 0.1 (random neighbours had 0.011: the restatement itself was 2e-5 from the fp64 value, the kernel 2e-6).  Here it is 0.44."""
    w = HW // 2 + 1 if resampled else HW
    g = torch.Generator().manual_seed(4000 + HW)
    gts, preds, masks = mg.random_inputs(g, 3, (1, HW), (1, w), "dense")
    p1 = mg.resample(preds[1, 0].numpy(), 1, HW)[0]
    gts[1, 0, 0, 0] = float(p1[0]) / 1.3
    gts[1, 0, 0, HW - 1] = float(p1[HW - 1]) * 1.2
    masks[0] = True
    masks[1] = False
    masks[1, 0, 0, 0] = masks[1, 0, 0, HW - 1] = True
    masks[2] = False
    masks[2, 0, 0, (HW - 1) // ED_CHUNK * ED_CHUNK:] = True
    return gts, preds, masks


@pytest.mark.parametrize("resampled", [False, True], ids=["identity", "resampled"])
@pytest.mark.parametrize("HW", [1, 255, 4095, 4096, 4097, 8193])
def test_pixel_counts_on_both_sides_of_the_chunk(HW, resampled):
    gts, preds, masks = _chunk_inputs(HW, resampled)
    ref, ns = mg.restate(gts, preds, masks)
    assert ns.tolist() == [HW, min(HW, 2), HW - (HW - 1) // ED_CHUNK * ED_CHUNK]
    got = _run(gts, preds, masks)
    for k in mg.KEYS:
        print(HW, resampled, k, got[k], ref[k])
    assert mg.compare(got, ref, ns) == []


# ---- ratios exactly on a threshold ----------------------------------------------------------------------------------------------------

DAUC_PICKED = tuple(range(0, 100, 11))     # ten of the hundred d_auc thresholds, both ends among them


def _threshold_inputs():
    """g = 1 and p > 1, so r = max(1 / p, p / 1) = p exactly whatever 1 / p rounds to.  p is every counting threshold and its fp32
    neighbour towards 1: image 0 holds all of them, image 1 only the values ON a threshold.  -> gts, preds, masks [2,1,1,n], thr, e"""
    from unidepth_amd import eval_ops
    th = eval_ops._dauc_thresholds(torch.device("cuda", torch.cuda.current_device())).cpu().numpy()      # the tensor the op reads
    thr, e = th[:100].copy(), th[100:].copy()
    on = np.array([1.25, 1.5625, 1.953125, np.float32(1.03)] + [thr[j] for j in DAUC_PICKED], np.float32)
    below = np.nextafter(on, np.float32(1.0))
    assert (below < on).all() and (below > 1.0).all() and len(set(on.tolist())) == len(on)
    p = np.concatenate([on, below])
    n = p.size
    assert n == 28 and n <= 200
    preds = torch.from_numpy(np.stack([p, p])).reshape(2, 1, 1, n)
    gts = torch.ones(2, 1, 1, n)
    masks = torch.ones(2, 1, 1, n, dtype=torch.bool)
    masks[1, 0, 0, n // 2:] = False
    return gts, preds, masks, thr, e


def test_ratios_exactly_on_a_threshold_are_not_counted():
    gts, preds, masks, thr, e = _threshold_inputs()
    got = _run(gts, preds, masks)
    for b in range(2):
        p = preds[b, 0, 0][masks[b, 0, 0]].numpy()
        n = p.size
        assert n == (28, 14)[b]
        for key, t in (("d1", 1.25), ("d2", 1.5625), ("d3", 1.953125), ("tau", np.float32(1.03))):
            count = int(np.count_nonzero(p < np.float32(t)))                      # strict: the value on the threshold is outside
            assert int(np.count_nonzero(p <= np.float32(t))) == count + 1         # .. and exactly one value sits on it
            want = np.float32(count) / np.float32(n)
            print(b, key, "count", count, "of", n, "got", got[key][b], "want", want)
            assert _bits(got[key][b:b + 1])[0] == _bits(np.array([want]))[0], (b, key, got[key][b], want)
        ref = mg.restate_one(np.ones(n, np.float32), p, thr=(thr, e))
        lax = mg.restate_one(np.ones(n, np.float32), np.nextafter(p, np.float32(1.0)), thr=(thr, e))     # what `<=` would count
        bound = float(lg.term_store_f32(torch.tensor(ref["d_auc"])))
        print(b, "d_auc", got["d_auc"][b], "restated", ref["d_auc"], "bound", bound, "with <=", lax["d_auc"])
        assert abs(lax["d_auc"] - ref["d_auc"]) > 100 * bound                     # the check separates < from <=
        assert abs(float(got["d_auc"][b]) - ref["d_auc"]) <= bound, (b, got["d_auc"][b], ref["d_auc"])


# ---- every radix digit in play --------------------------------------------------------------------------------------------------------

def _wide_inputs():
    """g log-uniform over [1e-3, 1e3], p = g exp(N(0, 1)): the keys of g and p spread over 20 binades (the top digit of the radix select
    takes ~10 values, every lower digit all 256), and d = ln p - ln g has both signs.  n = 5003 (odd) and 5002 (even)."""
    g = torch.Generator().manual_seed(77)
    n = 5003
    gts = torch.exp((torch.rand(2, 1, 1, n, generator=g) * 2 - 1) * float(np.log(1e3)))
    preds = gts * torch.exp(torch.randn(2, 1, 1, n, generator=g))
    masks = torch.ones(2, 1, 1, n, dtype=torch.bool)
    masks[1, 0, 0, 1234] = False
    return gts, preds, masks


def test_medians_when_every_radix_digit_differs():
    gts, preds, masks = _wide_inputs()
    ref, ns = mg.restate(gts, preds, masks)
    assert ns.tolist() == [5003, 5002]
    d = (torch.log(preds) - torch.log(gts)).numpy()
    assert (d > 0).mean() > 0.4 and (d < 0).mean() > 0.4
    top = np.unique(gts.numpy().view(np.uint32) >> 24).size
    assert top >= 8 and np.unique((gts.numpy().view(np.uint32) >> 16) & 255).size == 256
    got = _run(gts, preds, masks)
    for k in mg.KEYS:
        print(k, got[k], ref[k])
    assert mg.compare(got, ref, ns) == []


# ---- the C-ABI: guarded output, padded and dirty work area, no mask -------------------------------------------------------------------

def _cabi_inputs(hw):
    g = torch.Generator().manual_seed(4242)
    gts, preds, masks = mg.random_inputs(g, 3, (37, 53), hw, "dense")
    gts[0, 0, 5, 7] = float("nan")                                      # dropped by !(g <= max_depth)
    gts[1, 0, 0, 0] = 13.0                                              # > max_depth
    gts[2, 0, 36, 52] = float("inf")
    return gts, preds, masks


@pytest.mark.parametrize("hw", [(37, 53), (20, 31)], ids=["identity", "resampled"])
def test_cabi_guarded_with_a_dirty_work_area_and_no_mask(hw):
    gts, preds, masks = _cabi_inputs(hw)
    max_depth = 12.0
    assert int((gts > max_depth).sum()) > 3
    gt, pred = gts[:, 0].contiguous().cuda(), preds[:, 0].contiguous().cuda()
    ref, ns = mg.restate(gts, preds, torch.ones_like(masks), max_depth)
    assert all(0 < n < 37 * 53 for n in ns)
    clean = _cabi(gt, pred, None, max_depth, work_fill=0x00)
    for k in mg.KEYS:
        print(hw, k, clean[k], ref[k])
    assert mg.compare(clean, ref, ns) == []                             # mask = NULL with has_max_depth: an all-true mask
    assert _same_bits(_cabi(gt, pred, None, max_depth, work_fill=0xFF), clean)
    assert _same_bits(_cabi(gt, pred, None, max_depth, work_fill=0xA5, calls=2), clean)          # the second call meets the first one's state
    m8 = masks[:, 0].contiguous().cuda().view(torch.uint8)
    refm, nsm = mg.restate(gts, preds, masks, max_depth)
    withmask = _cabi(gt, pred, m8, max_depth, work_fill=0xFF, calls=2)
    assert mg.compare(withmask, refm, nsm) == []
    assert _same_bits(withmask, _run(gts, preds, masks, max_depth))     # the wrapper's call, bit for bit


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------

def test_wrapper_layouts_fp16_and_graph_replay_give_the_same_bits():
    from unidepth_amd import eval_ops
    g = torch.Generator().manual_seed(99)
    gts, preds, masks = (t.cuda() for t in mg.random_inputs(g, 2, (45, 70), (23, 31), "dense"))
    B, _, H, W = gts.shape
    h, w = preds.shape[-2:]
    ref = {k: v.cpu().numpy() for k, v in eval_ops.eval_depth(gts, preds, masks, max_depth=9.0).items()}
    g_nc = gts.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)                          # column-major memory
    wide = torch.zeros(B, 1, h, w + 9, device="cuda")
    wide[..., 4:4 + w] = preds
    p_nc = wide[..., 4:4 + w]                                                                # a column window of a wider tensor
    mwide = torch.zeros(B, 1, H + 3, W + 2, dtype=torch.bool, device="cuda")
    mwide[:, :, 1:1 + H, 2:] = masks
    m_nc = mwide[:, :, 1:1 + H, 2:]                                                          # a bool view
    assert not g_nc.is_contiguous() and not p_nc.is_contiguous() and not m_nc.is_contiguous()
    got = {k: v.cpu().numpy() for k, v in eval_ops.eval_depth(g_nc, p_nc, m_nc, max_depth=9.0).items()}
    assert _same_bits(got, ref)
    p16 = {k: v.cpu().numpy() for k, v in eval_ops.eval_depth(gts, preds.half(), masks, max_depth=9.0).items()}
    p16f = {k: v.cpu().numpy() for k, v in eval_ops.eval_depth(gts, preds.half().float(), masks, max_depth=9.0).items()}
    assert _same_bits(p16, p16f) and not _same_bits(p16, ref)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = eval_ops.eval_depth(gts, preds, masks, max_depth=9.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits({k: v.cpu().numpy() for k, v in cap.items()}, ref)
