"""Autograd functions of the training path: every forward AND backward is a HIP kernel launch (MFMA GEMMs for the
dense gradients, streaming kernels for the rest); torch.autograd only orders the calls and owns the saved tensors.

Conventions: activations that feed a GEMM are bf16 `[M, K]`; the residual stream and all parameter gradients are f32.
For Y = X W^T (X [M, K], W [N, K]):
    dX = dY W          -> NT GEMM with A = dY [M, N],   B = W^T [K, N]   (W^T packed once per weight version)
    dW = dY^T X        -> the same kernel with transposed operands (desc.trans_ab: dY and X read as they lie; `wgrad` below), or, for
                          shapes outside it, NT GEMM with A = dY^T [N, M], B = X^T [K, M] after tribe_transpose_bf16
    db = column sums of dY.
Reference semantics followed: pl_module.py:126-128 (training_step = _run_step loss -> Lightning backward),
model.py:113-174 (forward graph), x_transformers encoder (oracle/xt_encoder.py).
"""

from __future__ import annotations

import typing as tp

import torch

from tribe_hip import _lib, ops
from tribe_hip._lib import BF16, F32, ROLE, check, lib

_DT = {torch.float32: F32, torch.bfloat16: BF16}


_LOG2E = 1.4426950408889634


_s = ops._stream
_gemm = ops._gemm   # the one GEMM launcher (tribe_hip/ops.py)


def transpose_bf16(x: torch.Tensor, Z: int, R: int, Cc: int, s_z: int, s_r: int, off: int = 0) -> torch.Tensor:
    """out[z, c, r] = x[z, r, c] as bf16 [Z, C, R_pad64] (x f32 or bf16, strided view given by element strides / offset)."""
    R_pad = ops.round_up(R, 64)
    out = torch.empty(Z, Cc, R_pad, dtype=torch.bfloat16, device=x.device)
    check(lib().tribe_transpose_bf16(x.data_ptr() + x.element_size() * off, _DT[x.dtype], Z, R, Cc, s_z, s_r, out.data_ptr(), Cc * R_pad, R_pad,
                                     _s()), "tribe_transpose_bf16")
    return out


def grad_sums_and_cast(dy: torch.Tensor, M: int, N: int, res: torch.Tensor | None = None, want_sum: bool = False,
                       want_bf16: bool = True) -> tuple[torch.Tensor | None, torch.Tensor | None, torch.Tensor | None]:
    """One pass over an incoming f32 gradient dy [M, N]: (column sums or None, column sums of dy * res or None, bf16 copy or None) --
    the bias gradient, the res_scale gradient and the GEMM operand of a Linear / FeedForward backward (tribe_colsum_cast_fwd)."""
    dev = dy.device
    if dy.dtype != torch.float32 or N % 4:
        return (colsum(dy, M, N) if want_sum else None, colsum(dy, M, N, b=res) if res is not None else None,
                cast_bf16(dy) if want_bf16 else None)
    sa = torch.empty(N, dtype=torch.float32, device=dev) if want_sum else None
    sab = torch.empty(N, dtype=torch.float32, device=dev) if res is not None else None
    bf = torch.empty(M, N, dtype=torch.bfloat16, device=dev) if want_bf16 else None
    check(lib().tribe_colsum_cast_fwd(dy.data_ptr(), ops._p(res), M, N, N, ops._p(sa), ops._p(sab), ops._p(bf), N, _s()), "tribe_colsum_cast_fwd")
    return sa, sab, bf


# weight gradients may take the stream-K schedule of the transposed-operand GEMM (tribe_gemm_desc.stream_k).  The planner cuts only a last
# round that is at most half full: dW of a 12288 x 3072 layer (576 tiles = 2.25 rounds of 256 CUs) and of the 64-tile projectors are split,
# dW of a 3072 x 3072 layer (144 tiles) and of QKV (432) stay whole.  Split tiles are summed in a fixed order: bit-reproducible.
STREAM_K_WGRAD = True


def wgrad_reads_transposed(M: int, N: int, K: int, ld_dy: int, ld_x: int) -> bool:
    """Whether `wgrad` takes the transposed-operand form of the GEMM (stated once; tests/test_autograd_ref_host.py holds the copy in the
    case table of oracle/autograd_ref.py to it)."""
    return M % 64 == 0 and N % 8 == 0 and K % 8 == 0 and N >= 128 and K >= 128 and ld_dy % 8 == 0 and ld_x % 8 == 0


def wgrad(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, M: int, N: int, K: int, ld_dy: int, ld_x: int) -> None:
    """dw[n, k] = sum_m dy[m, n] x[m, k]  (dy bf16 [M, ld_dy >= N], x bf16 [M, ld_x >= K], dw f32 [N, K]): the weight gradient of a Linear.
    Shapes the 256^2 kernel covers go through its transposed-operand form (desc.trans_ab: dy and x are read as they lie, the LDS reads
    transpose); the rest keep the two explicit bf16 transposes in front of the NT GEMM."""
    if wgrad_reads_transposed(M, N, K, ld_dy, ld_x):
        _gemm(dy, x, dw, lda=ld_dy, ldb=ld_x, ldc=K, M=N, N=K, K=M, trans_ab=True, stream_k=STREAM_K_WGRAD)
        return
    dy_t = transpose_bf16(dy, 1, M, N, 0, ld_dy)[0]   # [N, M_pad]
    x_t = transpose_bf16(x, 1, M, K, 0, ld_x)[0]      # [K, M_pad]
    Mp = dy_t.shape[1]
    _gemm(dy_t, x_t, dw, lda=Mp, ldb=Mp, ldc=K, M=N, N=K, K=Mp)


def dense_bwd(dpre: torch.Tensor, x: torch.Tensor, wt: torch.Tensor, N: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(dx, dw) of y = x W^T from dpre = dy as bf16 [M, N]: x bf16 [M, K], wt = W^T bf16 [K, N_pad64] (the second half of a pack).
    dx is bf16 like x (autograd would cast an f32 gradient in a pass of its own), dw f32 [N, K]."""
    M, K = x.shape
    Np = wt.shape[1]
    if Np != N:
        dpre = torch.nn.functional.pad(dpre, (0, Np - N))  # zero K-padding for the dgrad GEMM (N % 64 != 0 only)
    dx = torch.empty(M, K, dtype=x.dtype, device=x.device)
    _gemm(dpre, wt, dx, lda=Np, ldb=Np, ldc=K, M=M, N=K, K=Np)
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device)
    wgrad(dpre, x, dw, M, N, K, Np, K)   # dW[n, k] = sum_m dpre[m, n] x[m, k]
    return dx, dw


def res_grad(dy: torch.Tensor, res: torch.Tensor, res_scale: torch.Tensor | None, raw: bool) -> torch.Tensor:
    """Gradient of the residual input of y = ... + res * res_scale from dy f32 [M, N]; raw: the residual came from ScaleNormFork,
    which applies res_scale to its gradient itself, so dy goes back as it is."""
    if raw:
        return dy
    dres = torch.empty_like(res)
    check(lib().tribe_scale_cols_fwd(dy.data_ptr(), ops._p(res_scale), dy.shape[0], dy.shape[1], dres.data_ptr(), _s()), "tribe_scale_cols_fwd")
    return dres


def upstream_scale(g: torch.Tensor) -> torch.Tensor:
    """The gradient arriving at a scalar loss as the f32 [1] device tensor its backward kernel reads."""
    return g.reshape(1).to(torch.float32).contiguous()


def colsum(a: torch.Tensor, M: int, N: int, b: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    acc = out is not None
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=a.device)
    check(lib().tribe_colsum_fwd(a.data_ptr(), _DT[a.dtype], ops._p(b), M, N, N, out.data_ptr(), int(acc), _s()), "tribe_colsum_fwd")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == torch.bfloat16:
        return x.contiguous()
    x = x.contiguous()
    if x.numel() % 4 and x.ndim == 2 and x.dtype == torch.float32:
        # the vector kernel takes multiples of 4; odd MLP shapes go through the row kernel's element path (no norm, no activation: a cast)
        return ops.norm_act(x, None, None, 0.0, None, norm=False, ld_out=x.shape[1])[0]
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().tribe_cast_bf16_fwd(x.data_ptr(), x.numel(), y.data_ptr(), _s()), "tribe_cast_bf16_fwd")
    return y


class _WeightPacks:
    """bf16 W [N, K_pad] and W^T [K_pad, N_pad] per (tensor object, version) of an f32 weight; entries die with the tensor
    (temporaries are rebuilt every step, parameters only when they were updated).  An unpadded pack (K % 64 == 0: a plain element-wise
    cast) is registered as the parameter's bf16 shadow (modeling_utils/shadow.py): HipAdam's kernel then writes it while it updates the
    parameter and `_refreshed` records the new version -- no cast pass after the step; W^T is re-derived from the bf16 pack."""

    def __init__(self) -> None:
        self._c: dict[int, list] = {}     # id(w) -> [weakref, sig, pack, packT]

    def _refreshed(self, key: int, w_ref: tp.Any, version: int) -> None:
        hit, w = self._c.get(key), w_ref()
        if hit is None or w is None or hit[0]() is not w:
            return
        hit[1] = (w.data_ptr(), version, tuple(w.shape))
        N, K = w.shape
        hit[3] = transpose_bf16(hit[2], 1, N, K, 0, hit[2].shape[1])[0]     # [K, N_pad64] from the fresh bf16 pack

    def get(self, w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        import weakref

        from . import shadow

        key = id(w)
        sig = (w.data_ptr(), w._version, tuple(w.shape))
        hit = self._c.get(key)
        if hit is None or hit[0]() is not w or hit[1] != sig:
            wd = w.detach().contiguous()
            N, K = wd.shape
            ref = weakref.ref(w, lambda _r, k=key: self._c.pop(k, None))
            hit = [ref, sig, ops.pack_weight(wd), transpose_bf16(wd, 1, N, K, 0, K)[0]]
            if hit[2].shape[1] != K:
                # a Linear behind K-padded activations (an MLP's hidden width that is no multiple of 64): its dgrad GEMM produces all
                # K_pad columns of dx and reads as many rows of W^T -- the rows past K are zeros, like the pad columns of the pack
                hit[3] = torch.cat([hit[3], hit[3].new_zeros(hit[2].shape[1] - K, hit[3].shape[1])])
            self._c[key] = hit
            if hit[2].shape == wd.shape and w.is_contiguous() and isinstance(w, torch.nn.Parameter):
                shadow.register(w, hit[2], lambda version, k=key, r=ref: self._refreshed(k, r, version))
        return hit[2], hit[3]


PACKS = _WeightPacks()


# ------------------------------------------------------------------------------------------------------------
class Linear(torch.autograd.Function):
    """y = x W^T + b (+ res * res_scale).  x bf16 [M, K]; W f32 [N, K]; y bf16 or f32 [M, N]."""

    @staticmethod
    def forward(ctx, x, w, b, res, res_scale, out_f32: bool, raw_res_grad: bool = False):
        ctx.raw_res_grad = raw_res_grad   # see res_grad
        M, K = x.shape
        N = w.shape[0]
        wp, _ = PACKS.get(w)
        Kp = wp.shape[1]
        if Kp != K:
            raise ValueError(f"Linear: activation width {K} must equal the packed K {Kp} (pad activations to 64)")
        y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
        _gemm(x, wp, y, lda=K, ldb=Kp, ldc=N, M=M, N=N, K=K, bias=b, res=res, res_scale=res_scale)
        ctx.save_for_backward(x, w, res, res_scale)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, res, res_scale = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        dy = dy.contiguous()
        dres = res_grad(dy, res, res_scale, ctx.raw_res_grad) if res is not None else None
        # bias gradient, res_scale gradient and the bf16 GEMM operand from ONE pass over dy
        db, drs, dpre = grad_sums_and_cast(dy, M, N, res=res if (res is not None and res_scale is not None) else None, want_sum=ctx.has_b)
        dx, dw = dense_bwd(dpre, x, PACKS.get(w)[1], N)
        dw = dw[:, : w.shape[1]] if w.shape[1] != K else dw
        return dx, dw, db, dres, drs, None, None


class _FusedQKVPacks:
    """bf16 [3N, K] (q | k | v rows) and its transpose [K, 3N] for one attention block, rebuilt only when one of the three f32
    weights was written: each weight is packed STRAIGHT into its row slice -- no f32 `torch.cat` of the three matrices per layer and
    step (113 MB written + read back, plus the split in backward), which model.py:228 of round 1 did.  The three row slices are the
    parameters' bf16 shadows (see _WeightPacks): after a HipAdam step only the transpose is re-derived."""

    def __init__(self) -> None:
        self._c: dict[int, list] = {}     # id(wq) -> [weakref, sig, fused, fusedT, [weak refs of the three weights]]

    def _refreshed(self, key: int, index: int, version: int) -> None:
        """HipAdam wrote the bf16 rows of weight `index` together with its f32 value, which now stands at `version`.  Only THAT
        weight's signature entry moves: a sibling written outside the optimiser (load_state_dict, copy_) that got no gradient in this
        step keeps its recorded version, still mismatches in get() and is repacked there."""
        hit = self._c.get(key)
        if hit is None:
            return
        ws = [r() for r in hit[4]]
        if any(w is None for w in ws) or hit[0]() is not ws[0]:
            return
        sig = list(hit[1])
        sig[index] = (ws[index].data_ptr(), version, tuple(ws[index].shape))
        hit[1] = tuple(sig)
        hit[3] = None                                                            # the transpose is re-derived on the next get()

    def get(self, ws: tuple[torch.Tensor, torch.Tensor, torch.Tensor]) -> tuple[torch.Tensor, torch.Tensor]:
        import weakref

        from . import shadow

        key = id(ws[0])
        sig = tuple((w.data_ptr(), w._version, tuple(w.shape)) for w in ws)
        hit = self._c.get(key)
        if hit is None or hit[0]() is not ws[0] or hit[1] != sig:
            N, K = ws[0].shape
            if any(tuple(w.shape) != (N, K) for w in ws) or K % 64:
                raise ValueError("fused q|k|v projection: the three weights must share one [N, K] shape with K % 64 == 0")
            fused = hit[2] if (hit is not None and hit[0]() is ws[0] and hit[2].shape == (3 * N, K)) else \
                torch.empty(3 * N, K, dtype=torch.bfloat16, device=ws[0].device)
            for i, w in enumerate(ws):
                wd = w.detach().contiguous()
                check(lib().tribe_pack_weight_bf16(wd.data_ptr(), N, K, K, fused[i * N:(i + 1) * N].data_ptr(), N, K, _s()), "tribe_pack_weight_bf16")
            hit = [weakref.ref(ws[0], lambda _r, k=key: self._c.pop(k, None)), sig, fused, None, [weakref.ref(w) for w in ws]]
            self._c[key] = hit
            for i, w in enumerate(ws):
                if isinstance(w, torch.nn.Parameter) and w.is_contiguous():
                    shadow.register(w, fused[i * N:(i + 1) * N], lambda version, k=key, i=i: self._refreshed(k, i, version))
        if hit[3] is None:
            N3, K = hit[2].shape
            hit[3] = transpose_bf16(hit[2], 1, N3, K, 0, K)[0]
        return hit[2], hit[3]


QKV_PACKS = _FusedQKVPacks()


class QKVLinear(torch.autograd.Function):
    """qkv = x [Wq; Wk; Wv]^T as ONE GEMM (x bf16 [M, K] -> bf16 [M, 3N]); backward: dx = dqkv W and ONE wgrad GEMM whose
    [3N, K] result is handed back as three row slices (views: no copy)."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv):
        M, K = x.shape
        N = wq.shape[0]
        wp, _ = QKV_PACKS.get((wq, wk, wv))
        y = torch.empty(M, 3 * N, dtype=torch.bfloat16, device=x.device)
        _gemm(x, wp, y, lda=K, ldb=K, ldc=3 * N, M=M, N=3 * N, K=K, role=ROLE["qkv"])
        ctx.save_for_backward(x, wq, wk, wv)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wq, wk, wv = ctx.saved_tensors
        N = wq.shape[0]
        _, wt = QKV_PACKS.get((wq, wk, wv))                     # [K, 3N_pad64]
        dx, dw = dense_bwd(cast_bf16(dy.contiguous()), x, wt, 3 * N)
        return dx, dw[:N], dw[N:2 * N], dw[2 * N:]


class FeedForward(torch.autograd.Function):
    """out = drop(gelu(x W1^T + b1)) W2^T + b2 + res * res_scale  (x_transformers FeedForward + scaled residual).
    x bf16 [M, D]; res f32 [M, D] (the block input); out f32 [M, D].  drop: ops.dropout_apply with (p, seed, site) on the bf16 hidden
    [M, Fh], in place between the two GEMMs; p == 0 (the default) launches nothing.  Backward: the same mask on dpre -- it commutes with
    the element-wise gelu' of the ACT_GELU_BWD epilogue -- and dW2 from the saved, dropped hidden."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, res, res_scale, raw_res_grad: bool = False, p: float = 0.0, seed: int = 0, site: int = 0):
        ctx.raw_res_grad = raw_res_grad   # see Linear
        ctx.drop = (float(p), int(seed), int(site))
        M, D = x.shape
        Fh = w1.shape[0]
        w1p, _ = PACKS.get(w1)
        w2p, _ = PACKS.get(w2)
        pre = torch.empty(M, Fh, dtype=torch.bfloat16, device=x.device)
        h = torch.empty(M, Fh, dtype=torch.bfloat16, device=x.device)
        _gemm(x, w1p, h, lda=D, ldb=D, ldc=Fh, M=M, N=Fh, K=D, bias=b1, act=_lib.ACT_GELU, aux=pre, role=ROLE["ff1"])
        if p > 0:
            ops.dropout_apply(h, p, seed, site, out=h)
        out = torch.empty(M, D, dtype=torch.float32, device=x.device)
        _gemm(h, w2p, out, lda=Fh, ldb=Fh, ldc=D, M=M, N=D, K=Fh, bias=b2, res=res, res_scale=res_scale, role=ROLE["ff2"])
        ctx.save_for_backward(x, w1, w2, pre, h, res, res_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, pre, h, res, res_scale = ctx.saved_tensors
        M, D = x.shape
        Fh = w1.shape[0]
        dout = dout.contiguous()
        dres = res_grad(dout, res, res_scale, ctx.raw_res_grad)
        db2, drs, dob = grad_sums_and_cast(dout, M, D, res=res if res_scale is not None else None, want_sum=True)   # one pass over dout
        _, w2t = PACKS.get(w2)                                  # [Fh, D]
        dpre = torch.empty(M, Fh, dtype=torch.bfloat16, device=x.device)
        _gemm(dob, w2t, dpre, lda=D, ldb=D, ldc=Fh, M=M, N=Fh, K=D, act=_lib.ACT_GELU_BWD, aux=pre)   # dh * gelu'(pre)
        if ctx.drop[0] > 0:
            ops.dropout_apply(dpre, *ctx.drop, out=dpre)
        dw2 = torch.empty(D, Fh, dtype=torch.float32, device=x.device)
        wgrad(dob, h, dw2, M, D, Fh, D, Fh)
        db1 = colsum(dpre, M, Fh)
        dx, dw1 = dense_bwd(dpre, x, PACKS.get(w1)[1], Fh)      # (no pad: ff_inner % 64 == 0)
        return dx, dw1, db1, dw2, db2, dres, drs, None, None, None, None


def _dg_buffers(rows: int, device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
    """(dg f32 [1], per-row staging f32 [rows]) of tribe_scalenorm_bwd_ordered: the gain gradient is the fixed-order sum of the rows' terms
    (the atomic sum of tribe_scalenorm_bwd differs in its last bits from run to run, which a seeded dropout run must not)."""
    return torch.empty(1, dtype=torch.float32, device=device), torch.empty(rows, dtype=torch.float32, device=device)


class ScaleNorm(torch.autograd.Function):
    """y = x / max(||x||, eps) * gain_scale * g  (bf16 out; x f32 [M, D])."""

    @staticmethod
    def forward(ctx, x, g, gain_scale: float, eps: float, out_f32: bool = False):
        y = ops.scalenorm(x, g, gain_scale, eps, torch.float32 if out_f32 else torch.bfloat16)
        ctx.save_for_backward(x, g)
        ctx.gs, ctx.eps = gain_scale, eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = dy.contiguous()
        M, D = x.shape
        dx = torch.empty_like(x)
        dg, dg_rows = _dg_buffers(M, x.device)
        check(lib().tribe_scalenorm_bwd_ordered(x.data_ptr(), dy.data_ptr(), _DT[dy.dtype], g.data_ptr(), ctx.gs, ctx.eps, M, D, None, None,
                                                dx.data_ptr(), dg.data_ptr(), dg_rows.data_ptr(), _s()), "tribe_scalenorm_bwd_ordered")
        return dx, dg, None, None, None


class ScaleNormFork(torch.autograd.Function):
    """(xn, xr) = (ScaleNorm(x), x): the input of a pre-norm block forked into its normed branch and its residual branch (x_transformers
    `Residual(scale_residual=True)`: block(norm(x)) + x * res_scale).  The backward adds the two incoming gradients INSIDE the ScaleNorm
    backward kernel, dx = d_norm + d_res * res_scale: the consumer of `xr` (Linear / FeedForward with raw_res_grad=True) hands its output
    gradient back as it is, so the per-block column scaling pass and autograd's add of the two branches (two f32 [M, D] passes each) go."""

    @staticmethod
    def forward(ctx, x, g, gain_scale: float, eps: float, res_scale):
        y = ops.scalenorm(x, g, gain_scale, eps, torch.bfloat16)
        ctx.save_for_backward(x, g, res_scale)
        ctx.gs, ctx.eps = gain_scale, eps
        # an unused branch arrives in backward as None, not as a zero tensor: without this line autograd materialised zeros, `dy is None` and
        # `dxr is None` below were never true, and a residual-only use ran the whole kernel over a zero gradient
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dxr):
        x, g, rs = ctx.saved_tensors
        M, D = x.shape
        if dy is None:    # the normed branch was not used: only the residual gradient flows
            dx = dxr if rs is None else dxr * rs
            return dx, None, None, None, None
        dx = torch.empty_like(x)
        dg, dg_rows = _dg_buffers(M, x.device)
        dy = dy.contiguous()
        dres = None if dxr is None else dxr.float().contiguous()
        check(lib().tribe_scalenorm_bwd_ordered(x.data_ptr(), dy.data_ptr(), _DT[dy.dtype], g.data_ptr(), ctx.gs, ctx.eps, M, D, ops._p(dres),
                                                None if dres is None else ops._p(rs), dx.data_ptr(), dg.data_ptr(), dg_rows.data_ptr(), _s()),
              "tribe_scalenorm_bwd_ordered")
        return dx, dg, None, None, None


_HeadSlice = tp.Tuple[torch.Tensor, int, int]


class _HeadGemms:
    """The batched per-(sequence, head) products of Attention for the sequences [b0, b0 + nb) of one chunk, each form stated once.
    A head slice of a row-major [B*T, ld] buffer is (tensor, ld, element offset of the chunk's first row, head 0): q / k / v build it for
    the column blocks of a fused [B*T, 3 * h * d] buffer (qkv, dqkv), o for a [B*T, h * d] one (out, dout).  A score buffer (S, P, dP, dS)
    is [sequences * h * T, Tp], Tp = T padded to 64."""

    def __init__(self, h: int, T: int, d: int, nb: int = 0, b0: int = 0) -> None:
        self.h, self.T, self.d, self.nb, self.Tp = h, T, d, nb, ops.round_up(T, 64)
        inner = h * d
        self.q, self.k, self.v = (lambda x, off=b0 * T * 3 * inner + i * inner: (x, 3 * inner, off) for i in range(3))
        self.o = lambda x: (x, inner, b0 * T * inner)
        self.rows = slice(b0 * h * T, (b0 + nb) * h * T)   # the chunk's rows (b, h, t) of the logical [B * h * T, T] scores, of lse and D
        self.n = nb * h * T                                # how many: the leading rows of a score buffer that the chunk uses
        self.s_scores = (h * T * self.Tp, T * self.Tp)     # batch strides (sequence, head) of a score buffer
        self.reads_transposed = T % 64 == 0 and d % 8 == 0   # dV, dK: `weighted_t` in place of `weighted`

    def chunk_size(self, B: int, score_bytes: int) -> int:
        """Sequences per chunk: one f32 score buffer stays within score_bytes."""
        return max(1, min(B, score_bytes // (self.h * self.T * self.Tp * 4)))

    def chunks(self, B: int, size: int) -> tp.Iterator[_HeadGemms]:
        return (_HeadGemms(self.h, self.T, self.d, min(size, B - b0), b0) for b0 in range(0, B, size))

    def score_buffer(self, size: int, dtype: torch.dtype, device: torch.device, zero_pad: bool = False) -> torch.Tensor:
        """For chunks of `size` sequences; zero_pad: the pad columns are zero from the start, for writers that leave them alone."""
        return (torch.zeros if zero_pad and self.Tp != self.T else torch.empty)(size * self.h * self.T, self.Tp, dtype=dtype, device=device)

    def _s_heads(self, ld: int) -> tuple[int, int]:
        return self.T * ld, self.d                         # batch strides (sequence, head) of a head slice

    def transposed(self, x: _HeadSlice) -> torch.Tensor:
        """A head slice as bf16 [nb * h, d, Tp] with zero pad columns: the second factor of `weighted`."""
        return _head_transpose(x[0], self.nb, self.h, self.T, self.d, x[1], x[2])

    def scores(self, a: _HeadSlice, b: _HeadSlice, out: torch.Tensor, alpha: float = 1.0, act: int = _lib.ACT_NONE,
               aux: torch.Tensor | None = None, row_bias: torch.Tensor | None = None) -> None:
        """out[(b, h), i, j] = act(alpha * sum_c a[b, i, h, c] * b[b, j, h, c] + row_bias[b, h, i]): two head slices -> a score buffer
        (q k^T, dO v^T).  aux: the score buffer `act` reads; row_bias: f32 over ALL logical rows [B * h * T], the chunk's are picked here."""
        (ta, lda, a_off), (tb, ldb, b_off) = a, b
        _gemm(ta, tb, out, lda=lda, ldb=ldb, ldc=self.Tp, M=self.T, N=self.T, K=self.d, alpha=alpha, act=act, aux=aux, ld_aux=self.Tp,
              batch1=self.nb, batch0=self.h, sA=self._s_heads(lda), sB=self._s_heads(ldb), sC=self.s_scores, a_off=a_off, b_off=b_off,
              row_bias=row_bias, row_bias_off=self.rows.start, sBias=(self.h * self.T, self.T))

    def weighted(self, w: torch.Tensor, xT: torch.Tensor, out: _HeadSlice) -> None:
        """out[b, i, h, :] = sum_j w[(b, h), i, j] x[b, j, h, :]: a score buffer times xT = transposed(x) -> a head slice.  The reduction
        runs along the ROWS of x, hence its per-(b, h) transposed copy [d, Tp]; K = Tp: the pad columns of both factors are zero."""
        to, ldc, c_off = out
        _gemm(w, xT, to, lda=self.Tp, ldb=self.Tp, ldc=ldc, M=self.T, N=self.d, K=self.Tp, batch1=self.nb, batch0=self.h, sA=self.s_scores,
              sB=(self.h * self.d * self.Tp, self.d * self.Tp), sC=self._s_heads(ldc), c_off=c_off)

    def weighted_t(self, w: torch.Tensor, x: _HeadSlice, out: _HeadSlice) -> None:
        """out[b, j, h, :] = sum_i w[(b, h), i, j] x[b, i, h, :] (where reads_transposed): both factors have the reduction index i on their
        ROWS -- the transposed-operand form of the GEMM (desc.trans_ab) reads the score buffer [T, Tp] and the head slice as they lie: no
        P^T, dS^T ([B h, T, T] each), q^T, dO^T."""
        (tx, ldx, x_off), (to, ldc, c_off) = x, out
        _gemm(w, tx, to, lda=self.Tp, ldb=ldx, ldc=ldc, M=self.T, N=self.d, K=self.T, batch1=self.nb, batch0=self.h, sA=self.s_scores,
              sB=self._s_heads(ldx), sC=self._s_heads(ldc), b_off=x_off, c_off=c_off, trans_ab=True)


class Attention(torch.autograd.Function):
    """softmax(q k^T * scale) v per (batch, head) on a fused bf16 qkv [B*T, 3*inner]; forward = fused flash kernel,
    backward = five MFMA GEMM products per head on P / dS recomputed per batch chunk.  Where the forward kernel can hand over its
    log-sum-exp (dim_head 384) the backward keeps no f32 [B h, T, T] tensor and runs no softmax kernel: the score GEMM's epilogue writes
    P = exp2(scale log2e q.k - lse2[row]) (ACT_EXP2), the dO V^T GEMM's epilogue writes dS = scale (dP - D[row]) * P (ACT_MUL_AUX) with
    D = rowsum(dO * O) (FlashAttention-2's identity for rowsum(P * dP)); 12 bytes of HBM traffic per score instead of 28.  Other head
    sizes (and FUSED_SOFTMAX = False) take the materialised S / dP + softmax kernels.

    Attention dropout (p > 0 with the pass key `seed` and the layer's `site`; x_transformers: attn = dropout(softmax(.)), out = attn v) never
    enters the flash kernel, at any head size.  Forward, per chunk of sequences: f32 scores S = scale q k^T, ops.softmax_dropout_fwd (Pd =
    softmax(S) * m as bf16, the row log-sum-exp of the undropped scores), O = Pd V; saved: qkv, out, lse -- no [B h, T, T] tensor outlives the
    forward and no mask tensor exists.  Backward: D = rowsum(dO * O) (the identity holds since O = Pd V), P rebuilt by the ACT_EXP2 epilogue,
    dPd = dO V^T in f32, ops.softmax_dropout_bwd (dS = scale P (m dPd - D); P overwritten by Pd = P m with the mask drawn again), then the three
    gradient GEMMs with Pd for dV.  The mask is indexed by (b, h, i, j) through each chunk's first logical row: chunking does not move it.
    p == 0 (the default) runs exactly the launches described above.

    causal=True (x_transformers' Decoder: keys j > query i masked before the softmax) takes that materialised route at EVERY p, p == 0 included
    (threshold 0, scale_keep 1), with ops.softmax_causal_fwd / ops.softmax_causal_bwd in place of the two row kernels: they compute the lower
    triangle only, write exact zeros above it and never read what the mask-unaware ACT_EXP2 epilogue left there.  The GEMMs still compute
    full squares (skipping their upper-triangle tiles is the GEMM's business).  causal=False launches what it always did."""

    # f32 score bytes per chunk of sequences.  Same box, B = 16 (scripts/train_bench.py attn-chunk=N): 7 sequences (256 MiB) 112.0 ms,
    # 4 sequences 110.9, 2 sequences 117.4, 1 sequence 122.5 -- smaller chunks keep more of S / P / dP / dS in the Infinity Cache but
    # leave the batched GEMMs under one round of tiles
    CHUNK_BYTES = 144 << 20
    # With the fused-softmax backward only P and dS (bf16) exist and fewer, larger batched GEMMs win: B = 16 in one chunk 102.8 ms, 8 sequences
    # 103.7, 4 sequences 104.5 (materialised path, 4 sequences: 105.8; same box, profiles/r03_z5_train.txt)
    CHUNK_BYTES_FUSED = 1 << 30
    FUSED_SOFTMAX = True

    @staticmethod
    def _fwd_masked(qkv, B: int, T: int, h: int, d: int, scale: float, drop: tuple[float, int, int], causal: bool):
        """(out, lse) of the materialised forward under a mask: attention dropout, the causal mask (at any p, 0 included) or both."""
        softmax_fwd = ops.softmax_causal_fwd if causal else ops.softmax_dropout_fwd
        dev = qkv.device
        heads = _HeadGemms(h, T, d)
        size = heads.chunk_size(B, Attention.CHUNK_BYTES)
        out = torch.empty(B * T, h * d, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, h, T, dtype=torch.float32, device=dev)
        S = heads.score_buffer(size, torch.float32, dev)
        Pd = heads.score_buffer(size, torch.bfloat16, dev)   # (the kernel zeroes the pad columns)
        for g in heads.chunks(B, size):
            g.scores(g.q(qkv), g.k(qkv), S, alpha=scale)
            softmax_fwd(S[:g.n], *drop, T=T, row0=g.rows.start, out=Pd[:g.n], lse=lse.view(-1)[g.rows])
            g.weighted(Pd, g.transposed(g.v(qkv)), g.o(out))   # O[q, :] = sum_key Pd[q, key] V[key, :]
        return out, lse

    @staticmethod
    def _fwd_any(ctx, qkv, B: int, T: int, heads: int, dim_head: int, scale: float, p: float, seed: int, site: int, causal: bool = False):
        """Runs the forward of the route and records it in ctx.route: "masked" (dropout and / or causal), "fused" (the flash kernel hands
        over its log-sum-exp) or "materialised"."""
        ctx.meta = (B, T, heads, dim_head, scale)
        ctx.drop = (float(p), int(seed), int(site))
        ctx.causal = bool(causal)
        if ctx.drop[0] > 0 or ctx.causal:
            ctx.route = "masked"
            out, lse = Attention._fwd_masked(qkv, B, T, heads, dim_head, scale, ctx.drop, ctx.causal)
            ctx.save_for_backward(qkv, out, lse)
        elif Attention.FUSED_SOFTMAX and ops.attention_lse_supported(dim_head):
            ctx.route = "fused"
            out, lse = ops.attention_with_lse(qkv, B, T, heads, dim_head, scale)
            ctx.save_for_backward(qkv, out, lse)
        else:
            ctx.route = "materialised"
            out = ops.attention(qkv, B, T, heads, dim_head, scale)
            ctx.save_for_backward(qkv)
        return out

    @staticmethod
    def forward(ctx, qkv, B: int, T: int, heads: int, dim_head: int, scale: float, p: float = 0.0, seed: int = 0, site: int = 0,
                causal: bool = False):
        out = Attention._fwd_any(ctx, qkv, B, T, heads, dim_head, scale, p, seed, site, causal)
        ctx.rotary = None
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, route = ctx.saved_tensors[0], ctx.route
        softmax_bwd = ops.softmax_causal_bwd if ctx.causal else ops.softmax_dropout_bwd
        B, T, h, d, scale = ctx.meta
        dev = qkv.device
        dout = cast_bf16(dout)
        dqkv = torch.empty_like(qkv)
        heads = _HeadGemms(h, T, d)
        Tp = heads.Tp
        size = heads.chunk_size(B, Attention.CHUNK_BYTES_FUSED if route == "fused" else Attention.CHUNK_BYTES)
        if route != "materialised":
            _, out, lse = ctx.saved_tensors
            neg_lse = lse.neg()                                      # the row bias of the ACT_EXP2 epilogue, [B, h, T] f32
            neg_d = ops.rowdot_heads(dout, out, B, T, h, d, -scale)  # -scale * D: the row bias of ACT_MUL_AUX, what the masked row kernel adds
        # the pad columns of P and dS, which the K = Tp products read, are zero: the row kernels write them (the causal one also everything
        # above the diagonal); the fused route's GEMMs write columns < T only and start from zeros
        P = heads.score_buffer(size, torch.bfloat16, dev, zero_pad=route == "fused")
        dS = heads.score_buffer(size, torch.bfloat16, dev, zero_pad=route == "fused")
        S = heads.score_buffer(size, torch.float32, dev) if route == "materialised" else None
        dP = heads.score_buffer(size, torch.float32, dev) if route != "fused" else None
        st = _s()
        for g in heads.chunks(B, size):
            if route == "materialised":
                g.scores(g.q(qkv), g.k(qkv), S, alpha=scale)         # S = scale * Q K^T ;  P = softmax(S)
                check(lib().tribe_softmax_fwd(S.data_ptr(), g.n, T, Tp, P.data_ptr(), Tp, Tp, st), "tribe_softmax_fwd")
                g.scores(g.o(dout), g.v(qkv), dP)                    # dP = dO V^T ;  dS = P * (dP - rowsum(P dP)) * scale
                check(lib().tribe_softmax_bwd(P.data_ptr(), dP.data_ptr(), g.n, T, Tp, Tp, Tp, scale, dS.data_ptr(), Tp, st), "tribe_softmax_bwd")
            else:
                # P = exp2(scale log2e Q K^T - lse2) straight out of the GEMM epilogue
                g.scores(g.q(qkv), g.k(qkv), P, alpha=scale * _LOG2E, act=_lib.ACT_EXP2, row_bias=neg_lse)
                if route == "fused":                                 # dS = (scale dO V^T - scale D) * P, out of the epilogue too
                    g.scores(g.o(dout), g.v(qkv), dS, alpha=scale, act=_lib.ACT_MUL_AUX, aux=P, row_bias=neg_d)
                else:   # dPd = dO V^T (f32), then dS = scale P (m dPd - D) and P <- Pd = P m in one row kernel
                    g.scores(g.o(dout), g.v(qkv), dP)
                    softmax_bwd(P[:g.n], dP[:g.n], neg_d.view(-1)[g.rows], scale, *ctx.drop, T=T, row0=g.rows.start, dS=dS[:g.n])
            g.weighted(dS, g.transposed(g.k(qkv)), g.q(dqkv))         # dQ[q, :] = sum_key dS[q, key] K[key, :]
            # dV[key, :] = sum_q P[q, key] dO[q, :] and dK[key, :] = sum_q dS[q, key] Q[q, :]  (P: Pd on the masked route)
            if g.reads_transposed:
                g.weighted_t(P, g.o(dout), g.v(dqkv))
                g.weighted_t(dS, g.q(qkv), g.k(dqkv))
            else:
                qT, doT = g.transposed(g.q(qkv)), g.transposed(g.o(dout))
                PT, dST = (transpose_bf16(x, g.nb * h, T, T, T * Tp, Tp) for x in (P, dS))
                g.weighted(PT, doT, g.v(dqkv))
                g.weighted(dST, qT, g.k(dqkv))
        if ctx.rotary is not None:   # RotaryAttention: rotate dq, dk back in place -- dqkv is this function's own buffer
            cos, neg_sin, rot_dim, interleaved = ctx.rotary
            ops.rotary_(dqkv, T, h, d, rot_dim, cos, neg_sin, interleaved)
        return (dqkv,) + (None,) * 9


class RotaryAttention(torch.autograd.Function):
    """Rotary (in place on the q and k heads of the fused qkv buffer) + attention as ONE node: the backward rotates dq, dk by -theta in the
    gradient buffer it allocated itself.  As two nodes (a rotary function in front of Attention) the rotation had to work on a clone of the incoming gradient
    (302 MB copied per layer and step at B = 16) and negate the sine table every call.  (p, seed, site): Attention's attention dropout;
    causal: Attention's mask."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, neg_sin, B: int, T: int, heads: int, dim_head: int, scale: float, rot_dim: int, interleaved: bool,
                p: float = 0.0, seed: int = 0, site: int = 0, causal: bool = False):
        ctx.mark_dirty(qkv)
        ops.rotary_(qkv, T, heads, dim_head, rot_dim, cos, sin, interleaved)
        out = Attention._fwd_any(ctx, qkv, B, T, heads, dim_head, scale, p, seed, site, causal)
        ctx.rotary = (cos, neg_sin, rot_dim, interleaved)
        return out, qkv

    @staticmethod
    def backward(ctx, dout, _dqkv_alias):
        return (Attention.backward(ctx, dout)[0],) + (None,) * 14


def _head_transpose(x: torch.Tensor, nb: int, h: int, T: int, d: int, ld: int, off: int) -> torch.Tensor:
    """[nb, T, (h, d)] strided view -> bf16 [nb*h, d, T_pad]: one launch, batch levels (sequence, head)."""
    Tp = ops.round_up(T, 64)
    out = torch.empty(nb * h, d, Tp, dtype=torch.bfloat16, device=x.device)
    check(lib().tribe_transpose_bf16_b2(x.data_ptr() + x.element_size() * off, _DT[x.dtype], nb, h, T, d, T * ld, d, ld, out.data_ptr(), d * Tp, Tp,
                                        _s()), "tribe_transpose_bf16_b2")
    return out


class VoxelHead(torch.autograd.Function):
    """SubjectLayers: y[b, v, t] = sum_c x[b, t, c] W[s_b, c, v] + bias[s_b, v].  x bf16 [B, T, C]; y f32 [B, V, T]."""

    @staticmethod
    def forward(ctx, x, w, bias, subjects):
        S, Cc, V = w.shape
        wp = ops.pack_subject_weights(w.detach().contiguous())
        y = ops.voxel_head(x, wp, None if bias is None else bias.detach().contiguous(), subjects, V)
        ctx.save_for_backward(x, w, subjects)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, subjects = ctx.saved_tensors
        B, T, Cp = x.shape
        S, Cc, V = w.shape
        dy = dy.contiguous()
        dev = x.device
        Vp, Tp = ops.round_up(V, 64), ops.round_up(T, 64)
        # dx[b, t, c] = sum_v dy[b, v, t] W[s_b, c, v]:  A = dy_b^T [T, Vp],  B = W[s_b] [C, Vp]
        dyT = ops.pack_features(dy, layer_mean=False, K_pad=Vp).view(B, T, Vp)            # "b v t -> b t v" + cast
        wv = ops.pack_weight(w.detach().reshape(S * Cc, V).contiguous(), cols_pad=Vp)     # [S*C, Vp]
        dx = torch.empty(B, T, Cp, dtype=torch.float32, device=dev)
        if Cp != Cc:
            dx.zero_()
        _gemm(dyT, wv, dx, lda=Vp, ldb=Vp, ldc=Cp, M=T, N=Cc, K=Vp, batch1=B, sA=(T * Vp, 0), sB=(Cc * Vp, 0), sC=(T * Cp, 0),
              gather1=subjects, gather_b=True)
        # dW[s, c, v] += sum_t x[b, t, c] dy[b, v, t]  for every sample b of subject s:  A = x_b^T [C, Tp], B = dy_b [V, Tp]
        xT = transpose_bf16(x, B, T, Cc, T * Cp, Cp)                                        # [B, C, Tp]
        dyb = ops.pack_weight(dy.reshape(B * V, T), cols_pad=Tp)                            # [B*V, Tp] bf16
        # one batched launch for the B per-sample products, then the samples of a subject summed in sample order on the device: no
        # device -> host read of `subjects` (it stalled the launch queue once per step) and B / 256-CU-filling tiles instead of B serial
        # 32-tile GEMMs chained through dW
        dw = torch.zeros(S, Cc, V, dtype=torch.float32, device=dev)
        if (Cc * V) % 4 == 0:
            dwb = torch.empty(B, Cc, V, dtype=torch.float32, device=dev)
            _gemm(xT, dyb, dwb, lda=Tp, ldb=Tp, ldc=V, M=Cc, N=V, K=Tp, batch1=B, sA=(Cc * Tp, 0), sB=(V * Tp, 0), sC=(Cc * V, 0))
            check(lib().tribe_slab_scatter_sum(dwb.data_ptr(), B, Cc * V, subjects.data_ptr(), dw.data_ptr(), _s()), "tribe_slab_scatter_sum")
        else:
            for b, s in enumerate(subjects.tolist()):
                _gemm(xT, dyb, dw, lda=Tp, ldb=Tp, ldc=V, M=Cc, N=V, K=Tp, a_off=b * Cc * Tp, b_off=b * V * Tp, c_off=s * Cc * V, res=dw,
                      ldres=V)
        db = None
        if ctx.has_bias:
            db = torch.zeros(S, V, dtype=torch.float32, device=dev)
            check(lib().tribe_rowsum_scatter(dy.data_ptr(), B, V, T, subjects.data_ptr(), db.data_ptr(), _s()), "tribe_rowsum_scatter")
        return dx, dw, db, None


class AdaptivePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t_out: int):
        ctx.t_in, ctx.t_out = x.shape[-1], t_out
        return ops.adaptive_avg_pool(x.contiguous(), t_out)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        rows = dy.numel() // ctx.t_out
        dx = torch.empty(*dy.shape[:-1], ctx.t_in, dtype=torch.float32, device=dy.device)
        check(lib().tribe_adaptive_avg_pool_bwd(dy.data_ptr(), rows, ctx.t_in, ctx.t_out, dx.data_ptr(), _s()), "tribe_adaptive_avg_pool_bwd")
        return dx, None


class ElemLoss(torch.autograd.Function):
    """ops.elem_loss (L1 / SmoothL1 / Huber / MSE, mean | sum) with its HIP backward; no gradient for the target."""

    @staticmethod
    def forward(ctx, pred, true, kind: str, param: float, reduction: str):
        pred, true = pred.contiguous(), true.contiguous()
        ctx.save_for_backward(pred, true)
        ctx.kind, ctx.param, ctx.reduction = kind, float(param), reduction
        return ops.elem_loss(pred, true, kind, param, reduction)

    @staticmethod
    def backward(ctx, g):
        pred, true = ctx.saved_tensors
        dp = torch.empty_like(pred)
        g = upstream_scale(g)
        check(lib().tribe_elem_loss_bwd(pred.data_ptr(), true.data_ptr(), pred.numel(), ops.ELEM_LOSS_KINDS[ctx.kind], ctx.param,
                                        ops.ELEM_LOSS_REDUCTIONS[ctx.reduction], g.data_ptr(), dp.data_ptr(), _s()), "tribe_elem_loss_bwd")
        return dp, None, None, None, None


class PearsonLossFn(torch.autograd.Function):
    """PearsonLoss over the '(b t) d' view of strided [B, V, T] tensors (losses.py:17-42)."""

    @staticmethod
    def forward(ctx, pred, true, reduction: str):
        out = ops.pearson_loss(pred, true, reduction)
        ctx.save_for_backward(pred, true)
        ctx.reduction = reduction
        return out

    @staticmethod
    def backward(ctx, g):
        pred, true = ctx.saved_tensors
        B, V, T = pred.shape
        sb, sv, st = pred.stride()
        stats = torch.zeros(1, V, 6, dtype=torch.float64, device=pred.device)
        ops.pearson_stats_update(stats, pred, true)
        dp = torch.empty(B, V, T, dtype=torch.float32, device=pred.device)
        g = upstream_scale(g)
        check(lib().tribe_pearson_loss_bwd(pred.data_ptr(), true.data_ptr(), B, V, T, sb, sv, st, stats.data_ptr(), int(ctx.reduction == "sum"),
                                           g.data_ptr(), dp.data_ptr(), _s()), "tribe_pearson_loss_bwd")
        if (sb, sv, st) != (V * T, T, 1):  # gradient in the layout of the (strided) input view
            dp = dp.as_strided((B, V, T), (V * T, T, 1))
            out = torch.empty_strided((B, V, T), (sb, sv, st), dtype=torch.float32, device=pred.device)
            out.copy_(dp)
            dp = out
        return dp, None, None


class InfoNCE(torch.autograd.Function):
    """Symmetric InfoNCE of model.py:208-221 on two [N, H] f32 latent matrices (rows are L2-normalised here)."""

    @staticmethod
    def forward(ctx, q, k, tau: float):
        N, H = q.shape
        dev = q.device
        one = torch.ones(1, dtype=torch.float32, device=dev)
        qn = ops.scalenorm(q.contiguous(), one, 1.0, 1e-12, torch.bfloat16)   # F.normalize(dim=-1)
        kn = ops.scalenorm(k.contiguous(), one, 1.0, 1e-12, torch.bfloat16)
        S = torch.empty(N, N, dtype=torch.float32, device=dev)
        St = torch.empty(N, N, dtype=torch.float32, device=dev)
        _gemm(qn, kn, S, lda=H, ldb=H, ldc=N, M=N, N=N, K=H, alpha=1.0 / tau)
        _gemm(kn, qn, St, lda=H, ldb=H, ldc=N, M=N, N=N, K=H, alpha=1.0 / tau)   # logits^T: its row LSE = column LSE of logits
        lse_r, lse_c, diag = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
        check(lib().tribe_lse_rows_fwd(S.data_ptr(), N, N, lse_r.data_ptr(), diag.data_ptr(), _s()), "tribe_lse_rows_fwd")
        check(lib().tribe_lse_rows_fwd(St.data_ptr(), N, N, lse_c.data_ptr(), None, _s()), "tribe_lse_rows_fwd")
        del St
        loss = 0.5 * ((lse_r - diag).mean() + (lse_c - diag).mean())  # two length-N vector reductions (host glue)
        ctx.save_for_backward(q, k, qn, kn, S, lse_r, lse_c)
        ctx.tau = tau
        return loss

    @staticmethod
    def backward(ctx, g):
        q, k, qn, kn, S, lse_r, lse_c = ctx.saved_tensors
        N, H = q.shape
        dev = q.device
        Np = ops.round_up(N, 64)
        gs = (g.reshape(1).to(torch.float32) / ctx.tau).contiguous()   # d logits / d (q.k) = 1 / tau
        dL = torch.empty(N, Np, dtype=torch.bfloat16, device=dev)
        check(lib().tribe_infonce_dlogits(S.data_ptr(), N, N, lse_r.data_ptr(), lse_c.data_ptr(), gs.data_ptr(), dL.data_ptr(), Np, _s()),
              "tribe_infonce_dlogits")
        knT = transpose_bf16(kn, 1, N, H, 0, H)[0]   # [H, Np]
        qnT = transpose_bf16(qn, 1, N, H, 0, H)[0]
        dLT = transpose_bf16(dL, 1, N, N, 0, Np)[0]  # [N, Np]
        dqn = torch.empty(N, H, dtype=torch.float32, device=dev)
        dkn = torch.empty(N, H, dtype=torch.float32, device=dev)
        _gemm(dL, knT, dqn, lda=Np, ldb=Np, ldc=H, M=N, N=H, K=Np)    # dq^ = dL k^
        _gemm(dLT, qnT, dkn, lda=Np, ldb=Np, ldc=H, M=N, N=H, K=Np)   # dk^ = dL^T q^
        one = torch.ones(1, dtype=torch.float32, device=dev)
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        for x, dy, dx in ((q, dqn, dq), (k, dkn, dk)):
            check(lib().tribe_scalenorm_bwd(x.data_ptr(), dy.data_ptr(), F32, one.data_ptr(), 1.0, 1e-12, N, H, None, None, dx.data_ptr(), None,
                                            _s()), "tribe_scalenorm_bwd")
        return dq, dk, None


class ProjectorFuse(torch.autograd.Function):
    """One modality's projector writing its column slice of the fused stream (+ positional / subject embeddings are
    added by EmbedAdd).  feat bf16 [M, Kp]; W f32 [N, K]; out slice f32 [M, N] (a fresh tensor; concat is done by cat)."""

    @staticmethod
    def forward(ctx, feat, w, b):
        M, Kp = feat.shape
        N = w.shape[0]
        wp, _ = PACKS.get(w)
        y = torch.empty(M, N, dtype=torch.float32, device=feat.device)
        _gemm(feat, wp, y, lda=Kp, ldb=Kp, ldc=N, M=M, N=N, K=Kp, bias=b, role=ROLE["projector"])
        ctx.save_for_backward(feat, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        feat, w = ctx.saved_tensors
        M, Kp = feat.shape
        N, K = w.shape
        dy = dy.contiguous()
        dyb = cast_bf16(dy)
        dw = torch.empty(N, Kp, dtype=torch.float32, device=feat.device)
        wgrad(dyb, feat, dw, M, N, Kp, N, Kp)
        return None, dw[:, :K].contiguous() if Kp != K else dw, colsum(dy, M, N) if ctx.has_b else None


class NormAct(torch.autograd.Function):
    """y = act(LayerNorm(z)) (norm=False: act(z)) between two Linear layers of an MLP: z f32 [M, N] (a Linear's output) -> bf16
    [M, N_pad64], pad columns zero: the next Linear's operand as it stands.  One row kernel each way (tribe_norm_act_fwd / _bwd); the
    backward takes the next Linear's bf16 dx and hands back f32 dz, dgamma and dbeta (fixed-order column sums)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, eps: float, act: str | None, norm: bool):
        z = z.contiguous()
        y, mean, rstd = ops.norm_act(z, gamma, beta, eps, act, norm=norm, want_stats=True)
        ctx.save_for_backward(z, mean, rstd, gamma, beta)
        ctx.act, ctx.norm = act, norm
        return y

    @staticmethod
    def backward(ctx, dy):
        z, mean, rstd, gamma, beta = ctx.saved_tensors
        want = ctx.norm and (gamma is not None or beta is not None) and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dz, dgamma, dbeta = ops.norm_act_bwd(dy if dy.stride(-1) == 1 else dy.contiguous(), z, mean, rstd, gamma, beta, ctx.act, norm=ctx.norm,
                                             param_grads=want)
        return dz, dgamma if gamma is not None else None, dbeta if beta is not None else None, None, None, None


class Dropout(torch.autograd.Function):
    """y = ops.dropout_apply(x, p, seed, site): x f32 or bf16 [M, W]; the mask covers the leading `dim` columns (default W; a K-padded
    operand [M, N_pad64] passes dim = N, its pad columns stay as they are).  Out of place by default.  inplace: x is overwritten and
    handed back (ctx.mark_dirty) -- only for a tensor no other function saved, such as NormAct's or Linear's fresh output.
    backward = dropout_apply(dy, same p / seed / site), a new tensor whose columns >= dim are zero."""

    @staticmethod
    def forward(ctx, x, p: float, seed: int, site: int, dim: int | None = None, inplace: bool = False):
        W = x.shape[1]
        dim = W if dim is None else int(dim)
        if not 0 < dim <= W:
            raise ValueError(f"Dropout: dim={dim} outside (0, {W}]")
        ctx.key, ctx.dim = (float(p), int(seed), int(site)), dim
        if inplace:
            ctx.mark_dirty(x)
            if p > 0:
                ops.dropout_apply(x[:, :dim], p, seed, site, out=x[:, :dim])
            return x
        x = x.contiguous()
        y = torch.empty_like(x) if dim == W else torch.zeros_like(x)
        ops.dropout_apply(x[:, :dim], p, seed, site, out=y[:, :dim])
        return y

    @staticmethod
    def backward(ctx, dy):
        dim = ctx.dim
        if dy.stride(-1) != 1:
            dy = dy.contiguous()
        dx = torch.empty_like(dy, memory_format=torch.contiguous_format) if dim == dy.shape[1] else \
            torch.zeros_like(dy, memory_format=torch.contiguous_format)
        ops.dropout_apply(dy[:, :dim], *ctx.key, out=dx[:, :dim])
        return dx, None, None, None, None, None


class PackRows(torch.autograd.Function):
    """x [M, K] (f32 or bf16) -> the bf16 [M, K_pad64] GEMM operand: f32 through tribe_pack_weight_bf16 (row-wise cast + zero padding), bf16
    as it lies when K % 64 == 0, else through tribe_pack_features with T = 1; the backward hands the leading K columns of the operand's
    gradient back in x's dtype."""

    @staticmethod
    def forward(ctx, x):
        ctx.k, ctx.dtype = x.shape[1], x.dtype
        x = x.contiguous()
        if x.dtype == torch.float32:
            return ops.pack_weight(x)
        return x if x.shape[1] % 64 == 0 else ops.pack_features(x.unsqueeze(-1), layer_mean=False)

    @staticmethod
    def backward(ctx, dy):
        return dy[:, : ctx.k].to(ctx.dtype)
