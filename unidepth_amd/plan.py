"""What the plan builders of UniDepthV2 (unidepthv2._Plan) and UniDepthV1 (unidepthv1._EncPlan / _EncPlanViT / _FullPlan) share: the
recorder base (launch program, device, packed weights, zeroed buffers, tap points, weight-name tags) and the ONE recording of the DINOv2
ViT encoder both families run.  A plan is recorded once per input signature and replayed by infer(); tools/plan_fingerprint.py pins
what these builders record."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .ops import UD_ACT_GELU, UD_EPI_F16, UD_EPI_F32, UD_EPI_QKV, UD_PICK_LARGE_TILE, UD_PICK_SCHEDULE
from .weights import _rup


class PlanRecorder:
    """A plan under construction.  Every tensor a recorded launch points to must stay referenced by the plan: `prog.keep` holds the
    tensors passed to a launch as tensors, an attribute has to hold whatever is only reached through a raw `data_ptr() + offset`."""

    def __init__(self, weights: dict, dev, P: Optional[ops.Program] = None):
        self.weights, self.dev = weights, dev
        self.prog = ops.Program() if P is None else P
        self.tap_points = []               # (name, number of ops after which it is valid, getter -> tensor in the reference's layout)
        self._wname = {id(v): k for k, v in weights.items() if torch.is_tensor(v)}

    def z(self, *shape, dtype=torch.float16):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def tap(self, name, fn):
        self.tap_points.append((name, len(self.prog), fn))

    def gemm(self, **kw):
        """prog.gemm; a GEMM recorded without a tag is tagged with the name of its packed weight (bench.py's per-class breakdown and
        profiles/*ops_per_launch.tsv join on these tags)."""
        if "tag" not in kw and id(kw.get("W")) in self._wname:
            kw["tag"] = self._wname[id(kw["W"])]
        return self.prog.gemm(**kw)

    # ---------------- DINOv2 ViT encoder (dinov2.py:306-347; block.py:84-109; attention.py:51-62; mlp.py:35-41)
    def vit_embed(self, patches, pos, cls_row, B, hw, D, tag=None):
        """Patch-embed GEMM (+ position embedding) into the fp32 token stream [B * Np, D] and the class-token row in front of every image."""
        from .unidepthv1 import _wk        # (imported here: unidepthv1 imports this module)
        w, Np = self.weights, _rup(hw + 1, 16)
        x = self.z(B * Np, D, dtype=torch.float32)
        self.gemm(A=patches, W=w["patch.w"], bias=w["patch.b"], out=x, add=pos, M=B * hw, N=D, lda=640, ldc=D, ldadd=D, epi=UD_EPI_F32,
                  rows_in=hw, rows_out=Np, row_off=1, add_row_off=1, **_wk(w["patch.w"], 640), **({"tag": tag} if tag else {}))
        self.prog.fill_rows(x, cls_row, B, Np, 0, D, D)
        return x

    def vit_blocks(self, x, B, hw, arch, *, prefix, ln_tag=None, alias_hid=False, allow_fold=True, algo_flops=False, hook):
        """The `depth` blocks on the token stream x: (LN, qkv, attention, proj, LN, fc1 + GELU, fc2) per block, seven launches -- five where
        the LayerNorms are folded.  K / ldw / a_wrap of every GEMM come from the packed weight (unidepthv1._wk: V1 stores two fp16 terms).
        prefix: of the launch tags (`enc.` / `vit.`); ln_tag: tag of the LayerNorm launches (None: the kernel class); alias_hid: Q|K and the
        attention output live inside the MLP's hidden buffer; allow_fold: the caller's policy on top of the fold's eligibility (below);
        algo_flops: record the algorithmic flops of the unpadded token count in prog.meta instead of the GEMM's own M * N * K;
        hook(i, where, x, qk, vt): called after the qkv GEMM (where = "qkv") and at the end (where = "end") of block i.
        Returns (fold, tickets): whether the LayerNorms were folded, and the producers' ticket words (None where the weights carry no wsum)."""
        from .unidepthv1 import _wk
        w, P, z = self.weights, self.prog, self.z
        D, depth, heads = arch["D"], arch["depth"], arch["heads"]
        f32 = torch.float32
        N = hw + 1
        Np = _rup(N, 16)              # token rows per image (16: V^T block order of the QKV epilogue)
        Nkp = _rup(N, 64)
        M = B * Np
        xn, vt, hid = z(M, D), z(B, heads, 64, Nkp), z(M, 4 * D)
        if alias_hid:
            # Q|K and the attention output live inside `hid`: between fc2 of block i and fc1 of block i+1 the hidden activations are dead, and
            # q|k / ao are dead while fc1 / fc2 run.  The block's working set drops from 272 MB to 204 MB at bs = 8 (ViT-L) -- under the 256 MB
            # Infinity Cache, so what one launch writes the next one reads on-die (tools/r4_insitu.py: the step's launches ran 36 us per block
            # behind the same launches on warm operands).  V^T keeps its own buffer: its pad columns must stay zero.
            flat = hid.view(-1)
            qk = flat[: M * 2 * D].view(M, 2 * D)
            ao = flat[M * 2 * D: M * 3 * D].view(M, D)
        else:
            qk, ao = z(M, 2 * D), z(M, D)
        # LayerNorm folded into the neighbouring GEMMs (UdGemm.row_stats_out / row_stats_in): proj / fc2 write the raw fp16 copy of the
        # residual stream and per-row partial sums with their fp32 accumulate, qkv / fc1 normalise in their epilogues -- no LayerNorm
        # launch, no second pass over x.  Only where the packed weights carry the row sums (`enc.*.wsum`: V1's packer stores none) and all
        # four GEMMs run on the large-tile kernel (its epilogues hold the statistics code): bs >= 4 or so for ViT-L; smaller problems keep
        # the LayerNorm kernel.
        fold, tickets, slabs = False, None, D // 64
        if "enc.0.qkv.wsum" in w:
            x16 = z(M, D)
            rpart = z(M, slabs, 2, dtype=f32)                           # per 64-column slab (sum, sum of squares) written by proj / fc2
            rstats = z(M, 2, dtype=f32)                                 # (rstd, -mean * rstd) per row, reduced by the producer's last workgroup per row tile
            tickets = torch.zeros(2, M // 128 + 2, dtype=torch.int32, device=self.dev)     # one set per producer (proj, fc2): a set counts arrivals of ONE tiling
            big = all(ops.gemm_pick(A=xn, W=w[f"enc.0.{nm}.w"], out=xn, M=M, N=n_, K=k_, lda=k_, ldw=k_, ldc=n_, epi=e_, vsplit=2 * D, tok_per_img=Np,
                                    kv_ld=Nkp, heads_v=heads, out2=vt, accumulate=int(e_ == UD_EPI_F32),
                                    **(dict(row_stats_in=rstats, wsum=w[f"enc.0.{nm}.wsum"]) if nm in ("qkv", "fc1") else {})) & UD_PICK_SCHEDULE in UD_PICK_LARGE_TILE
                      for nm, n_, k_, e_ in (("qkv", 3 * D, D, UD_EPI_QKV), ("proj", D, D, UD_EPI_F32), ("fc1", 4 * D, D, UD_EPI_F16), ("fc2", D, 4 * D, UD_EPI_F32)))
            fold = big and allow_fold
            lnc = dict(row_stats_in=rstats, ln_slabs=slabs, ln_D=D, ln_eps=1e-6)
            prod = dict(out2=x16, ldc2=D, row_stats_out=rpart, row_stats_final=rstats, row_stats_ticket=tickets[0], ln_D=D, ln_eps=1e-6)
        fl = {k: dict(flops=c * B * N * D * D) for k, c in (("qkv", 6.0), ("proj", 2.0), ("fc1", 8.0), ("fc2", 8.0))} if algo_flops else {}
        ln = dict(x=x, y=xn, rows=M, D=D, ldx=D, ldy=D, eps=1e-6, rows_per_img=M, in_rows_per_img=M, out_rows_per_img=M, **({"tag": ln_tag} if ln_tag else {}))

        def lin(i, nm, K, **kw):            # one GEMM of block i on its packed weight
            self.gemm(W=w[f"enc.{i}.{nm}.w"], bias=w[f"enc.{i}.{nm}.b"], M=M, lda=K, tag=prefix + nm, **_wk(w[f"enc.{i}.{nm}.w"], K), **fl.get(nm, {}), **kw)

        for i in range(depth):
            folded = fold and i > 0            # block 0 reads what the embedding wrote: no producer has left statistics yet
            if not folded:
                P.layernorm(**ln)
            lin(i, "qkv", D, A=x16 if folded else xn, out=qk, out2=vt, N=3 * D, ldc=2 * D, epi=UD_EPI_QKV, vsplit=2 * D, tok_per_img=Np, kv_ld=Nkp,
                heads_v=heads, **(dict(wsum=w[f"enc.{i}.qkv.wsum"], **lnc) if folded else {}))
            hook(i, "qkv", x, qk, vt)
            P.attention(Q=qk, K=qk.data_ptr() + D * 2, Vt=vt, O=ao, B=B, H=heads, Nq=N, Nk=N, ldq=2 * D, ldk=2 * D, ldo=D,
                        kv_ld=Nkp, q_rows_per_img=Np, k_rows_per_img=Np, scale=(D // heads) ** -0.5, q_prescaled=1, tag=prefix + "attn")
            lin(i, "proj", D, A=ao, out=x, N=D, ldc=D, epi=UD_EPI_F32, accumulate=1, **(prod if fold else {}))
            if not fold:
                P.layernorm(**ln)
            lin(i, "fc1", D, A=x16 if fold else xn, out=hid, N=4 * D, ldc=4 * D, epi=UD_EPI_F16, act=UD_ACT_GELU,
                **(dict(wsum=w[f"enc.{i}.fc1.wsum"], **lnc) if fold else {}))
            last = i == depth - 1                                        # nothing consumes the last block's raw copy
            lin(i, "fc2", 4 * D, A=hid, out=x, N=D, ldc=D, epi=UD_EPI_F32, accumulate=1,
                **(dict(prod, row_stats_ticket=tickets[1]) if fold and not last else {}))
            hook(i, "end", x, qk, vt)
        return fold, tickets
