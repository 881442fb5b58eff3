"""What the depth-pyramid tests share (not a test module): the numpy fp32 restatement of csrc/pyramid_point.h, the scenes, and the call of
the host program tests/pyramid_host/pyramid_host.cpp.  The restatement is the first oracle of the GPU tests; the second is
unidepth_amd.pyramid.depth_pyramid_composition."""
import functools

import numpy as np

import host_program
from host_program import f32_bits, same_bits  # noqa: F401  (the tests reach them through this module)

F = np.float32
NB = 256
FLT_MAX = F(3.402823466e38)
INF_BITS = 0x7F800000


def tables(radius, sigma_space, sigma_range):
    """the filter's tables in fp64 numpy, rounded to fp32 once: what prepare_depth_filter must upload -> (ws, wr, inv_bin)"""
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    ws = np.exp(-(ax[None, :] ** 2 + ax[:, None] ** 2) / (2.0 * sigma_space ** 2)).reshape(-1)
    step = 3.0 * sigma_range / NB
    wr = np.exp(-(((np.arange(NB) + 0.5) * step) ** 2) / (2.0 * sigma_range ** 2))
    wr[NB - 1] = 0.0
    return ws.astype(F), wr.astype(F), F(1.0 / step)


def restate(depth, levels, *, mask=None, weights=None, radius=0, ws=None, wr=None, inv_bin=None, gate=np.inf, stats=None):
    """csrc/pyramid_point.h on a batch, every operation one fp32 numpy operation in the header's order.  depth fp32 [B,H,W], mask uint8
    [B,H,W], weights fp32 [B,H,W] -> ([depth_l], [weights_l] or None).  stats: a dict that receives `last_bin` (the share of the used
    taps of live centres that fall in bin NB - 1) and `gated` (the share of the level-1 blocks with a live member that exclude at least
    one live member through the gate)."""
    d = np.ascontiguousarray(depth, F)
    B, H, W = d.shape
    gate = F(gate)
    with np.errstate(all="ignore"):
        live = (d > 0) & (d <= FLT_MAX)
        if mask is not None:
            live &= np.asarray(mask) != 0
        if weights is not None:
            w = np.ascontiguousarray(weights, F)
            live &= (w > 0) & (w <= FLT_MAX)
        staged = np.where(live, d, F(0)).astype(F)
        r = radius
        if r == 0:
            level = staged
        else:
            padded = np.zeros((B, H + 2 * r, W + 2 * r), F)
            padded[:, r:r + H, r:r + W] = staged
            num, den = np.zeros_like(staged), np.zeros_like(staged)
            k = 2 * r + 1
            taps = last = 0
            for dy in range(k):
                for dx in range(k):
                    t = padded[:, dy:dy + H, dx:dx + W]
                    used = (t > 0) & live
                    delta = np.abs(t - staged).astype(F)
                    q = (delta * F(inv_bin)).astype(F)
                    idx = np.where(q >= F(NB), F(NB - 1), np.where(used, q, F(0))).astype(np.int64)
                    wt = (ws[dy * k + dx] * wr[idx]).astype(F)
                    num = np.where(used, (num + (wt * t).astype(F)).astype(F), num)
                    den = np.where(used, (den + wt).astype(F), den)
                    taps += int(used.sum())
                    last += int((used & (idx == NB - 1)).sum())
            level = np.where(live, (num / np.where(live, den, F(1))).astype(F), F(0)).astype(F)
            if stats is not None:
                stats["last_bin"] = last / max(taps, 1)
        out_d = [level]
        out_w = None if weights is None else [np.where(live, w, F(0)).astype(F)]
        for l in range(1, levels):
            prev = out_d[-1]
            h, wd = prev.shape[1] // 2, prev.shape[2] // 2
            mem = [prev[:, i:2 * h:2, j:2 * wd:2] for i in (0, 1) for j in (0, 1)]
            any_live, anchor = np.zeros(mem[0].shape, bool), np.zeros(mem[0].shape, F)
            for m in mem:
                lv = m > 0
                anchor = np.where(lv & (~any_live | (m < anchor)), m, anchor)
                any_live |= lv
            inc = [(m > 0) & ((m - anchor).astype(F) <= gate) for m in mem]
            n = np.zeros(mem[0].shape, np.int64)
            total = np.zeros(mem[0].shape, F)
            for m, i in zip(mem, inc):
                total = np.where(i, np.where(n > 0, (total + m).astype(F), m), total)
                n = n + i
            fn = np.where(n > 0, n, 1).astype(F)
            out_d.append(np.where(n > 0, (total / fn).astype(F), F(0)).astype(F))
            if l == 1 and stats is not None:
                n_live = sum((m > 0).astype(np.int64) for m in mem)
                stats["gated"] = float(((n < n_live) & any_live).sum()) / max(int(any_live.sum()), 1)
            if out_w is not None:
                pw = out_w[-1]
                wm = [pw[:, i:2 * h:2, j:2 * wd:2] for i in (0, 1) for j in (0, 1)]
                k, wt = np.zeros(mem[0].shape, np.int64), np.zeros(mem[0].shape, F)
                for m, i in zip(wm, inc):
                    wt = np.where(i, np.where(k > 0, (wt + m).astype(F), m), wt)
                    k = k + i
                out_w.append(np.where(n > 0, (wt / fn).astype(F), F(0)).astype(F))
    return out_d, out_w


# ---- the scenes --------------------------------------------------------------------------------------------------------------------

SIGMA_SPACE, SIGMA_RANGE, GATE = 1.5, 0.02, 0.08       # with the scenes' noise of 0.05 both gates decide both ways (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def scene(B, H, W, seed=0):
    """a step edge (2.0 left of a slanted line, 2.6 right of it) under a ramp and noise of 0.05, with holes (0), a mask that drops a tenth
    of the pixels and weights in 0.5 .. 2 of which a twentieth are 0 -> dict(depth, mask, weights)"""
    g = np.random.RandomState(4100 + seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.where(x + 0.3 * y < 0.55 * (W + 0.3 * H), 2.0, 2.6) + 0.002 * x
    depth = (base[None] + 0.05 * g.standard_normal((B, H, W))).astype(F)
    depth[g.uniform(size=(B, H, W)) < 0.05] = 0
    mask = (g.uniform(size=(B, H, W)) > 0.1).astype(np.uint8)
    weights = np.where(g.uniform(size=(B, H, W)) > 0.05, g.uniform(0.5, 2.0, size=(B, H, W)), 0).astype(F)
    return dict(depth=depth, mask=mask, weights=weights)


def step_scene(H, W):
    """a clean vertical step edge between 1.0 and 4.0 in the middle column, no noise: with the gate below the step no block of any level
    may hold a value between the two surfaces"""
    depth = np.where(np.arange(W)[None, :] < W // 2 + 1, 1.0, 4.0).astype(F).repeat(H, 0).reshape(1, H, W)
    return dict(depth=depth, mask=None, weights=None)


def special_scene():
    """NaN, +-inf, negatives, -0, subnormals and huge values in the depth and the weights, next to ordinary pixels: B = 2 images of 8 x 12.
    With the tables of sigma_range 1e-3 (inv_bin about 8.5e4) the product delta * inv_bin overflows to +inf next to the 1e38 pixels."""
    s = scene(2, 8, 12, seed=7)
    d, w, m = s["depth"].copy(), s["weights"].copy(), s["mask"].copy()
    d[0].reshape(-1)[:12] = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e38, 1e-40, 1e-38, 3e38, 1e-45, 2.0]
    d[1, 3, 3:7] = [1e38, 1e-3, 3.3e38, 1e38]
    w[0].reshape(-1)[12:20] = [np.nan, np.inf, -1.0, 0.0, -0.0, 1e-40, 3e38, 1e-45]
    w[1, 3, 3:7] = [3e38, 3e38, 3e38, 3e38]
    m[0, 0, :] = 1
    m[1, 3, :] = 1
    return dict(depth=d, mask=m, weights=w)


# ---- the host program --------------------------------------------------------------------------------------------------------------

def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "pyramid_host")


def level_sizes(H, W, levels):
    return [(H >> l, W >> l) for l in range(levels)]


def host_run(exe, depth, levels, *, mask=None, weights=None, radius=0, ws=None, wr=None, inv_bin=None, gate=np.inf):
    """the host program on a batch -> ([depth_l], [weights_l] or None)"""
    d = np.ascontiguousarray(depth, F)
    B, H, W = d.shape
    args = [B, H, W, levels, radius, int(mask is not None), int(weights is not None), f32_bits(float(gate)),
            f32_bits(float(inv_bin)) if radius else 0]
    blobs = [d.tobytes()]
    blobs += [np.ascontiguousarray(mask, np.uint8).tobytes()] if mask is not None else []
    blobs += [np.ascontiguousarray(weights, F).tobytes()] if weights is not None else []
    blobs += [np.ascontiguousarray(ws, F).tobytes(), np.ascontiguousarray(wr, F).tobytes()] if radius else []
    sizes = [4 * B * h * w for h, w in level_sizes(H, W, levels)]
    out = host_program.run(exe, args, blobs, sizes * (2 if weights is not None else 1))
    maps = [np.frombuffer(o, F).reshape((B,) + hw) for o, hw in zip(out, level_sizes(H, W, levels) * 2)]
    return maps[:levels], (maps[levels:] if weights is not None else None)
