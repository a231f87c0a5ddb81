"""StackedBLSTMCNN on the MI355X kernels (models/CNNBLSTM/model.py:16-108).

The module keeps the reference's constructor (a YAML config path), its
submodule tree (encoder / lstm / projection / decoder as nn.Sequential /
nn.LSTM / nn.Linear, so state_dict keys and torch's default initialisation --
including the RNG draw order -- are identical to the reference), and its
forward/reconstruct_spectrogram semantics.  Only the arithmetic moves: the
forward is four autograd Functions whose forward AND backward launch the
libainp kernels:

  _ConvStackFn  conv3x3 (+BatchNorm2d+ReLU) blocks; each BN+ReLU is applied
                inside the next conv's input load, the encoder's last block is
                written straight into the LSTM's [N, T, C*F] layout
                (model.py:34-44,70-74 / 53-61,87)
  _BLSTMFn      nn.LSTM(bidirectional, batch_first): one MFMA GEMM per layer
                for both directions' input projections + the register-resident
                recurrence kernel (model.py:46-47,77)
  _ProjFn       nn.Linear(2H, 16F) written directly as the decoder's
                [N, 16, F, T] input (model.py:50,80-83)
  _L1Pow10LossFn the training loss of models/CNNBLSTM/train.py:70,104

BatchNorm statistics are optionally all-reduced across data-parallel ranks
through `comm` (SyncBN), so a DP run matches the single-process reference.
"""
from __future__ import annotations

import atexit
import os

import torch
import torch.nn as nn
import yaml

from . import ops


def load_config(config_path):
    """models/CNNBLSTM/model.py:10-14."""
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def _allreduce(comm, t):
    if comm is not None:
        comm.allreduce_sum_(t)
    return t


# ------------------------------------------------------------------ conv stack
class _ConvStackFn(torch.autograd.Function):
    """Sequence of Conv2d(3x3,p1) [+ BatchNorm2d + ReLU] blocks.

    spec: list of (has_bn, bn_module_or_None) per block; params: per block
    (w, b[, gamma, beta]).  out_ntcf: final BN+ReLU output written [N,W,C*H].
    """

    @staticmethod
    def forward(ctx, x, spec, training, out_ntcf, comm, bf16, l0_box, defer_wgrad, *params):
        N, _, H, W = x.shape
        saved_y = []
        affine = []          # per BN block: (scale, shift, save or None)
        act = (None, None)   # prologue for the next conv
        h = x
        pi = 0
        # SyncBN: the local element count rides in the all-reduced sums (sums[2C]),
        # so ranks with uneven shards still normalise with the global count
        count = N * H * W
        count_dev = None
        # bf16 configuration: pre-BN outputs in bf16 storage (the next conv's
        # forward / weight gradient and the BatchNorm passes read them) where
        # this conv and its consumer have the kernels for it
        ws_, q = [], 0
        for has_bn, _ in spec:
            ws_.append(params[q])
            q += 4 if has_bn else 2
        l0_path = bool(spec) and l0_box is not None and _l0_bf16_ok(
            (N, ws_[-1].shape[0], H, W))
        # activation layout per block: (input channel-last, output channel-last)
        lays = _cl_layouts(ws_, N, H, W, out_ntcf, x.shape[1])
        nbt = []             # num_batches_tracked += 1, applied by one multi-tensor add
        for bi, (has_bn, bn) in enumerate(spec):
            w, b = params[pi], params[pi + 1]
            pi += 2
            want_stats = has_bn and training
            y16 = False
            if bf16 and Y16 and has_bn and ops.io16_ok(N, w.shape[1], w.shape[0], H, W):
                if bi + 1 < len(spec):
                    wn = ws_[bi + 1]
                    y16 = ops.io16_ok(N, wn.shape[1], wn.shape[0], H, W)
                else:
                    y16 = l0_path          # the bf16 bridge to the LSTM reads it
            xcl, ycl = lays[bi]
            y, stats = ops.conv3x3_fwd(h, w, b, act[0], act[1], want_stats=want_stats, bf16=bf16,
                                       y16=y16, xcl=xcl, ycl=ycl)
            saved_y.append(y)
            if has_bn:
                gamma, beta = params[pi], params[pi + 1]
                pi += 2
                if training:
                    C = w.shape[0]
                    rm = bn.running_mean if bn.track_running_stats else None
                    rv = bn.running_var if bn.track_running_stats else None
                    mom = bn.momentum if bn.momentum is not None else 0.1
                    if comm is not None:
                        sums = _allreduce(comm, ops.bn_stats_reduce(stats, C, count=count))
                        count_dev = sums[2 * C:]
                        sc, sh, sv = ops.bn_finalize(sums, 0, gamma, beta, rm, rv, mom, bn.eps)
                    else:
                        # one launch: partials -> scale / shift / running statistics
                        sc, sh, sv = ops.bn_reduce_finalize(stats, C, count, gamma, beta, rm, rv,
                                                            mom, bn.eps)
                    if bn.track_running_stats:
                        nbt.append(bn.num_batches_tracked)
                else:
                    sc, sh = ops.bn_eval_affine(gamma, beta, bn.running_mean,
                                                bn.running_var, bn.eps)
                    sv = None
                affine.append((sc, sh, sv))
                act = (sc, sh)
            else:
                affine.append(None)
                act = (None, None)
            h = y
        if nbt:
            torch._foreach_add_(nbt, 1)
        last = affine[-1]
        yl = saved_y[-1]
        ylcl = lays[-1][1] if lays else False        # the last block's y channel-last
        yshape = (N, ws_[-1].shape[0], H, W)
        if last is not None and l0_box is not None and _l0_bf16_ok(yshape):
            # bf16 configuration: the LSTM's layer-0 operands are written as bf16
            # X / X^T for the bf16-operand GEMMs (gemm16.hip); the fp32 NTCF
            # tensor is never materialised -- autograd gets a stride-0
            # placeholder of its shape, and its gradient (dX, fp32) as usual
            if ylcl:
                # B16_KM: the backward reads X k-major, so no X^T is written
                # and H % 8 == 0: the chunked (data-parallel) weight gradient
                # reads 16-byte aligned gate-column views dg16[:, d*4H + r0:]
                km = ops.B16_KM and (N * W) % 32 == 0 and l0_box.get("H", 0) % 8 == 0
                l0_box["x16"] = ops.bn_relu_apply_ntcf_cl(yl, last[0], last[1], out32=False,
                                                          out16=True, outT=not km)[1]
                l0_box["km"] = km
            else:
                l0_box["x16"] = ops.bn_relu_apply_ntcf_bf16(yl, last[0], last[1])
            Nl, Cl, Hl, Wl = yshape
            out = torch.zeros((), device=yl.device).expand(Nl, Wl, Cl * Hl)
        elif last is not None and ylcl:
            out = ops.bn_relu_apply_ntcf_cl(yl, last[0], last[1])[0]
        elif last is not None:
            out = ops.bn_relu_apply(yl, last[0], last[1], ntcf=out_ntcf)
        else:
            out = yl
        ctx.spec = spec
        ctx.lays = lays
        ctx.bf16 = bf16
        # the stack input is the fp32 output projection's result, whose x6r
        # backward reads its gradient as [C*F, N*T]: dx written that way
        ctx.gx_cfnt = bool(getattr(x, "_ainp_cfnt_grad", False))
        # (mode, sink): mode False / True (side stream now) / "queue" (released at
        # the first BPTT); sink = the data-parallel GradAllReducer or None
        ctx.defer_wgrad, ctx.sink = defer_wgrad if isinstance(defer_wgrad, tuple) \
            else (defer_wgrad, None)
        ctx.param_objs = params
        ctx.out_ntcf = out_ntcf
        ctx.comm = comm
        ctx.count = count
        ctx.count_dev = count_dev     # global count (device) under SyncBN
        ctx.affine = affine
        ctx.save_for_backward(x, *saved_y, *params)
        ctx.nblocks = len(spec)
        return out

    @staticmethod
    def backward(ctx, g):
        nb = ctx.nblocks
        tensors = ctx.saved_tensors
        x = tensors[0]
        ys = tensors[1:1 + nb]
        params = tensors[1 + nb:]
        # parameter index of each block
        idx, pi = [], 0
        for has_bn, _ in ctx.spec:
            idx.append(pi)
            pi += 4 if has_bn else 2
        grads = [None] * len(params)
        g = g.contiguous()
        gx = None
        pre_sums = None   # the next block's BatchNorm reduce, fused into this dgrad
        pend = None       # (dy, w) of a data gradient the next apply recomputes
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        for bi in range(nb - 1, -1, -1):
            has_bn, _ = ctx.spec[bi]
            p0 = idx[bi]
            w = params[p0]
            y = ys[bi]
            xcl, ycl = ctx.lays[bi]
            if has_bn:
                sc, sh, sv = ctx.affine[bi]
                ntcf = ctx.out_ntcf and bi == nb - 1
                if pre_sums is None:
                    pre_sums = ops.bn_relu_bwd_reduce(g, y, sc, sh, sv, ntcf, cl=ycl)
                sums, pre_sums = _allreduce(ctx.comm, pre_sums), None
                cnt = ctx.count
                if ctx.count_dev is not None:
                    sums, cnt = torch.cat([sums, ctx.count_dev]), 0
                if (FUSE_BNA0 and bi == 0 and ycl and not ntcf and not ctx.needs_input_grad[0]
                        and WGRAD_LAST_MAIN and ctx.sink is None and tuple(w.shape[:2]) == (16, 1)
                        and g.dtype == torch.float32 and y.dtype == torch.float32):
                    # round 6: the first conv's weight gradient forms its dy from
                    # g and y itself (ops.conv3x3_wgrad_bnapply): gy, whose only
                    # consumer it is, is never written or read back
                    dw, db, dgam, dbet = ops.conv3x3_wgrad_bnapply(
                        x, None, None, g, y, sc, sh, params[p0 + 2], sv, sums, cnt)
                    grads[p0], grads[p0 + 1], grads[p0 + 2], grads[p0 + 3] = dw, db, dgam, dbet
                    continue
                # bf16 configuration: gy in bf16 storage where this conv's data
                # and weight gradients take it (they round it to bf16 anyway)
                gy16 = ctx.bf16 and GY16 and ops.dy16_ok(N, w.shape[1], w.shape[0], H, W)
                if pend is not None:   # dx of the 16 -> 1 conv recomputed into the apply
                    gy, dgam, dbet = ops.conv3x3_dgrad_bnapply(pend[0], pend[1], y, sc, sh,
                                                               params[p0 + 2], sv, sums, cnt,
                                                               gy16=gy16)
                    pend = None
                else:
                    gy, dgam, dbet = ops.bn_relu_bwd_apply(g, y, sc, sh, params[p0 + 2], sv, sums,
                                                           cnt, ntcf, gy16=gy16, cl=ycl)
                grads[p0 + 2], grads[p0 + 3] = dgam, dbet
            else:
                gy = g.view_as(y) if g.shape != y.shape else g
            if bi > 0:
                prev = ctx.affine[bi - 1]
                xin = ys[bi - 1]
                pro = (prev[0], prev[1]) if prev is not None else (None, None)
            else:
                xin = x
                pro = (None, None)
            # layouts: the conv's input xin (xcl), its output / gy (ycl)
            lw = dict(xcl=xcl, gcl=ycl)
            # the first conv's weight gradient is the backward's last work: with no
            # input gradient to compute, the main stream would only wait for it,
            # so it runs there, beside the side stream's tail (single process)
            last_main = (WGRAD_LAST_MAIN and bi == 0 and not ctx.needs_input_grad[0]
                         and ctx.sink is None)
            if last_main:
                dw, db = ops.conv3x3_wgrad(xin, gy, pro[0], pro[1], bf16=ctx.bf16, **lw)
            elif ctx.defer_wgrad == "queue":
                # off the critical path: queued, launched on the side stream when
                # the BPTT recurrence (64 workgroups) starts -- filling the CUs
                # it leaves idle (see _Deferred)
                Cout, Cin = w.shape[0], w.shape[1]
                dw = torch.empty(Cout, Cin, 3, 3, device=gy.device)
                db = torch.empty(Cout, device=gy.device)
                # the queue holds aliases only: autograd's AccumulateGrad steals a
                # gradient tensor nobody else references instead of cloning it
                # (a clone would copy it before the side stream writes it)
                dwv, dbv = _alias(dw), _alias(db)
                pr, bf = pro, ctx.bf16
                _Deferred.push(gy.device, lambda xin=xin, gy=gy, pr=pr, dwv=dwv, dbv=dbv, bf=bf,
                               lw=lw: ops.conv3x3_wgrad(xin, gy, pr[0], pr[1], bf16=bf,
                                                        out=(dwv, dbv), **lw),
                               (xin, gy) + tuple(t for t in pro if t is not None), (dwv, dbv),
                               params=ctx.param_objs[p0:p0 + 2], sink=ctx.sink,
                               first=min(Cout, Cin) <= 2)
            elif ctx.defer_wgrad:
                # off the critical path: on the side stream, overlapping the next
                # (HBM-bound) BatchNorm backward passes
                # ENC_SIDE2: the encoder's inner weight gradients (all but the
                # last block's) on the second side stream, so they do not queue
                # behind the 32 -> 64 one on the first
                k = 1 if (_enc_side2(ctx.bf16) and bi < nb - 1) else 0
                with _side_work(gy.device, k=k) as sw:
                    dw, db = ops.conv3x3_wgrad(xin, gy, pro[0], pro[1], bf16=ctx.bf16, **lw)
                    sw.handoff((xin, gy) + tuple(t for t in pro if t is not None), (dw, db))
                    # data parallel: all-reduced from the side stream as soon as
                    # they exist (the collective waits for this stream only).
                    # The collective's Work keeps a reference to what it reduces,
                    # so autograd gets a separate non-view alias of the same
                    # storage: AccumulateGrad then steals its tensor instead of
                    # cloning it on the compute stream before the side stream
                    # has written it (the BLSTM / _Deferred pattern)
                    _reduce_side(ctx.sink, ctx.param_objs[p0:p0 + 2], (dw, db))
                    dw, db = _alias(dw), _alias(db)
            else:
                dw, db = ops.conv3x3_wgrad(xin, gy, pro[0], pro[1], bf16=ctx.bf16, **lw)
            grads[p0], grads[p0 + 1] = dw, db
            if (bi > 0 and xcl and DGRAD_BNR and ctx.spec[bi - 1][0]
                    and ctx.affine[bi - 1][2] is not None):
                # dx channel-last into a BatchNorm+ReLU: its backward reduce
                # is summed by the data gradient's epilogue
                psc, psh, psv = ctx.affine[bi - 1]
                if (FUSE_BNA6 and not ycl and ys[bi - 1].dtype == torch.float32
                        and ops.dgrad_bnr_nodx_ok(gy, w, ys[bi - 1], bf16=ctx.bf16, xcl=ycl)):
                    # round 6: Conv2d(16, 1) -- the sums now, dx recomputed by the
                    # apply (ops.conv3x3_dgrad_bnapply, which takes dy [N, 1, H, W]
                    # and an fp32 y): never written or read back
                    _, pre_sums = ops.conv3x3_dgrad_bnr(gy, w, ys[bi - 1], psc, psh, psv,
                                                        bf16=ctx.bf16, xcl=ycl, want_dx=False)
                    g, pend = None, (gy, w)
                else:
                    g, pre_sums = ops.conv3x3_dgrad_bnr(gy, w, ys[bi - 1], psc, psh, psv,
                                                        bf16=ctx.bf16, xcl=ycl)
            elif (bi == 0 and ctx.needs_input_grad[0] and ctx.gx_cfnt and not xcl
                  and ops.dgrad_cfnt_ok(N, w.shape[1], w.shape[0], H, W)):
                # round 6: dx as [C, F, N, T] (an [N, C, F, T] view of it) --
                # _ProjFn._backward_x6's operand without the transposing copy
                gx = ops.conv3x3_dgrad(gy, w, bf16=ctx.bf16, xcl=ycl, cfnt=True)
            elif bi > 0 or ctx.needs_input_grad[0]:
                # dx in this conv's input layout (the previous block's y)
                g = ops.conv3x3_dgrad(gy, w, bf16=ctx.bf16, xcl=ycl, ycl=xcl)
                if bi == 0:
                    gx = g
        return (gx, None, None, None, None, None, None, None, *grads)


# Round 6: the decoder's last conv (16 -> 1): its data gradient only sums the
# BatchNorm reduce of decoder.5, and that layer's apply recomputes it
# (AINP_FUSE_BNA6=0: dx written and read back)
FUSE_BNA6 = os.environ.get("AINP_FUSE_BNA6", "1") != "0"


# Round 6: the encoder's first conv (1 -> 16) weight gradient with its
# BatchNorm+ReLU backward apply fused in (AINP_FUSE_BNA0=0: the apply pass
# writes gy, the strip weight gradient reads it)
FUSE_BNA0 = os.environ.get("AINP_FUSE_BNA0", "1") != "0"


# Round 6: the decoder's input gradient written [C, F, N, T] by its first
# conv's data gradient, the layout the fp32 projection backward reads
# (AINP_PROJ_CFNT=0: NCHW, transposed by a copy there)
PROJ_CFNT = os.environ.get("AINP_PROJ_CFNT", "1") != "0"


# Round 5: a data gradient feeding a BatchNorm+ReLU with channel-last
# activations also sums that BatchNorm's backward reduce in its epilogue
# (ops.conv3x3_dgrad_bnr; AINP_DGRAD_BNR=0: the separate reduce pass)
DGRAD_BNR = os.environ.get("AINP_DGRAD_BNR", "1") != "0"


# Round 5: channel-last activations ([N, F, T, C]) between the convs of both
# conv stacks (AINP_CL=0: NCHW everywhere, as before).  The projection's
# 16-channel decoder input stays NCHW (the GEMM writes it); 1-channel tensors
# are the same in either layout.
CL = os.environ.get("AINP_CL", "1") != "0"
# the encoder's 64-channel output channel-last too (AINP_CL_BRIDGE=0: NCHW,
# bridged by the NCHW <-> NTCF kernels)
CL_BRIDGE = os.environ.get("AINP_CL_BRIDGE", "1") != "0"


def _cl_layouts(ws, N, H, W, out_ntcf, cin0):
    """[(input channel-last, output channel-last)] per conv of a stack whose
    weights are ws: block i's output layout is block i+1's input layout."""
    nb = len(ws)
    if not (CL and nb and all(ops.cl_ok(N, w.shape[1], w.shape[0], H, W) for w in ws)):
        return [(False, False)] * nb
    outs = []
    for i, w in enumerate(ws):
        cout = w.shape[0]
        last = i == nb - 1
        # channel-last where a consumer conv reads it, and for the encoder's
        # 64-channel output (the channel-last NTCF bridge, bn.hip); the
        # decoder's 1-channel output is the same either way
        outs.append((not last and cout > 1) or (last and out_ntcf and cout == 64 and CL_BRIDGE))
    lays = []
    for i in range(nb):
        xin_cl = outs[i - 1] if i > 0 else False   # stack input: NCHW (or 1 channel)
        lays.append((xin_cl, outs[i]))
    del out_ntcf, cin0
    return lays


# the encoder's first-conv weight gradient on the main stream when nothing
# else is left there (AINP_WGRAD_LAST_MAIN=0: on the side stream, A/B)
WGRAD_LAST_MAIN = os.environ.get("AINP_WGRAD_LAST_MAIN", "1") != "0"
# bf16 configuration: BatchNorm-backward outputs in bf16 storage (AINP_GY16=0:
# fp32, as before; the conv results are the same bit for bit)
GY16 = os.environ.get("AINP_GY16", "1") != "0"
# bf16 configuration: pre-BatchNorm conv outputs in bf16 storage (AINP_Y16,
# on by default since round 5: with channel-last activations the C3-shape
# step measured 8.92 -> 8.48 ms/step with it; round 4's NCHW kernels had
# measured it slower, 9.60 -> 9.67).  Unlike gy this is a rounding point of
# its own: the BatchNorm statistics and the BatchNorm+ReLU that feeds the next
# conv see the bf16 values (autocast's bf16 conv output);
# tests/golden/gen_golden_r04.py rounds there too (meta/emu_y16 in its fixture).
Y16 = os.environ.get("AINP_Y16", "1") == "1"


def _l0_bf16_ok(y):
    """Shapes the bf16 layer-0 operand path supports (ainp_bn_relu_apply_ntcf_bf16,
    ainp_gemm_bf16nt): C*F % 64 == 0, even T, N*T % 8 == 0 (k-contiguous rows
    of 16 bytes for the weight-gradient GEMM).  Otherwise the fp32-staged bf16
    GEMM loop runs.  y: the encoder output or its (N, C, F, T) shape."""
    N, C, F, T = y if isinstance(y, tuple) else y.shape
    return (C * F) % 64 == 0 and T % 2 == 0 and (N * T) % 8 == 0


# ------------------------------------------------------------------ BLSTM
class _BLSTMFn(torch.autograd.Function):
    """nn.LSTM(I, H, L, batch_first=True, bidirectional=True) forward/backward.
    params: nn.LSTM's _flat_weights order, per layer
    (w_ih, w_hh, b_ih, b_hh, w_ih_rev, w_hh_rev, b_ih_rev, b_hh_rev)."""

    @staticmethod
    def forward(ctx, x, H, L, bf16, sink, l0_box, *params):
        N, T, I = x.shape
        NT = N * T
        x16 = l0_box.get("x16") if l0_box is not None else None
        inp = x.reshape(NT, I) if x16 is None else x.new_empty(0)
        saved = []
        h = None
        ctx.l016 = None
        ctx.l016_km = False
        for l in range(L):
            wf, hf, bif, bhf, wr, hr, bir, bhr = params[8 * l:8 * l + 8]
            Il = inp.shape[1] if (l > 0 or x16 is None) else I
            zx = torch.empty(N, T, 8 * H, device=x.device, dtype=torch.float32)
            if l == 0 and x16 is not None:
                # bf16-operand layer-0 projection: X (bf16 [NT, I]) x W_cat^T, both
                # directions in one GEMM (W_cat = [W_ih; W_ih_rev] as bf16)
                X16, XT16 = x16
                ctx.l016_km = bool(l0_box.get("km", False))
                W16 = torch.empty(8 * H, I, device=x.device, dtype=torch.bfloat16)
                WT16 = torch.empty(I, 8 * H, device=x.device, dtype=torch.bfloat16)
                ops.cast_bf16_t(wf, out=W16[:4 * H], outT=WT16[:, :4 * H])
                ops.cast_bf16_t(wr, out=W16[4 * H:], outT=WT16[:, 4 * H:])
                ops.gemm_bf16nt(X16.view(NT, I), W16, out=zx.view(NT, 8 * H),
                                bias=(bif, bhf, bir, bhr), bias_nsplit=4 * H,
                                nsplit=ops.b16_proj_split(NT, 8 * H, I))
                # the weight gradient's X operand: X^T [I, NT], or X [NT, I] k-major
                ctx.l016 = (X16.view(NT, I) if ctx.l016_km else XT16, WT16)
            elif (l == 0 and not bf16 and not ops.GEMM_EXACT
                  and ops.x6_256_eligible(NT, 8 * H, Il, 4 * H)):
                # fp32 layer-0 projection (360 GFLOP at C2) on the 256 x 256 tile
                (ops.gemm_x6r_nt if ops.X6R_FWD else ops.gemm_x6nt_256)(
                    inp, wf, wr, zx.view(NT, 8 * H), bias=(bif, bhf, bir, bhr), bias_nsplit=4 * H)
            else:
                ops.gemm(NT, 4 * H, Il, [inp, inp], Il, 1, [wf, wr], 1, Il,
                         [zx, zx[:, :, 4 * H:]], 8 * H, 1, bias1=[bif, bir], bias2=[bhf, bhr],
                         bf16=bf16)
            h, gates, cell = ops.lstm_rec_fwd(zx, hf, hr, H)
            saved += [inp, h, gates, cell]
            inp = h.view(NT, 2 * H)
        ctx.H, ctx.L, ctx.bf16 = H, L, bf16
        ctx.I = I
        # data parallel: the layer-0 input weights' gradients (89 % of the
        # gradient bytes, produced late) are handed to the reducer chunk by chunk
        ctx.sink = sink
        ctx.wih0 = (params[0], params[4])     # the Parameters themselves
        ctx.param_objs = params
        ctx.save_for_backward(*saved, *params)
        return h

    @staticmethod
    def backward(ctx, dh):
        H, L, bf16 = ctx.H, ctx.L, ctx.bf16
        ctx.early_done = False
        st = ctx.saved_tensors
        saved, params = st[:4 * L], st[4 * L:]
        dh = dh.contiguous()
        N, T, _ = dh.shape
        NT = N * T
        grads = [None] * len(params)
        gwi_of = {}                       # layer -> the pair's [dW_ih, dW_ih_rev]
        dx = None
        # The weight/bias gradients of layer l depend only on its gate
        # gradients, so they run on a side stream while the main stream goes
        # on with dX and layer l-1's recurrence (64 workgroups: most CUs idle).
        main = torch.cuda.current_stream(dh.device)
        # the BLSTM's weight gradients: on their own side stream (BLSTM_SIDE2),
        # so they start right behind their recurrence instead of queueing
        # behind the deferred decoder weight gradients
        side = _side_stream(dh.device, 1 if _blstm_side2(bf16) else 0)
        # data parallel: the side stream's weight / bias gradients are
        # all-reduced from the side stream as they are produced, so the compute
        # stream never waits for them (AccumulateGrad stores non-view aliases)
        dp_side = ctx.sink is not None and ctx.sink.early_ok and \
            getattr(ctx.sink, "side_ok", True) and all(p.grad is None for p in ctx.param_objs)
        main_first = ops.MAIN_FIRST

        def main_dx(l, dg2, inp, Il, wf, wr, l016, pair, to_sink, dg16, dgT16=None,
                    pair16=False):
            """Layer l's data gradient (and, for the layer-0 pair -- fp32 x6r or
            bf16 -- dW_ih) on the current stream; (dxi or None, [gW_ih,
            gW_ih_rev] or None)."""
            gwi = None
            dxi = None
            if pair or pair16:
                # the deferred decoder / projection weight gradients run beside
                # the pair; joining both side streams first was slower at C2
                # 
                dxi = torch.empty(NT, Il, device=dh.device)
                if pair:
                    gwi = [torch.empty(4 * H, Il, device=dh.device) for _ in range(2)]
                    ops.lstm_l0_bwd_x6(dg2, wf, wr, inp, dxi, gwi[0], gwi[1])
                else:
                    # bf16: dW_cat beside dX on the 256 x 256 tile, one launch
                    gcat = torch.empty(8 * H, Il, device=dh.device)
                    ops.lstm_l0_bwd_bf16(dg16, dgT16, l016[1], l016[0], dxi, gcat,
                                         km=ctx.l016_km)
                    gwi = [gcat[:4 * H], gcat[4 * H:]]
                if to_sink:
                    # all-reduced from the current stream right behind the pair;
                    # the reducer's Work holds these buffers, autograd gets None
                    for d in range(2):
                        ctx.sink.reduce_chunk(ctx.wih0[d], gwi[d], kind="pair")
                        ctx.wih0[d].grad = gwi[d]
            if not (l > 0 or ctx.needs_input_grad[0]):
                return dxi, gwi
            # dX = dg_f W_ih + dg_r W_ih_rev.  Layer 0 (Il = 16448: 10836
            # tiles) sums both directions inside each tile; the upper layers
            # (Il = 256: 168 tiles) write 4 K-slabs (two per direction,
            # 672 tiles) summed in fixed order.
            if pair or pair16:
                pass                                                  # dxi from the pair
            elif l016 is not None:
                dxi = ops.gemm_bf16nt(dg16, l016[1])                 # dg [NT,8H] x W_cat
            elif Il >= 1024:
                dxi = torch.empty(NT, Il, device=dh.device)
                ops.gemm(NT, Il, 4 * H, [dg2, dg2[:, 4 * H:]], 8 * H, 1, [wf, wr], Il, 1,
                         [dxi, dxi], Il, 1, ksplit=True, bf16=bf16)
            else:
                hk = 2 * H                      # half of a direction's 4H gate columns
                sl = torch.empty(4, NT, Il, device=dh.device)
                ops.gemm(NT, Il, hk, [dg2[:, q * hk:] for q in range(4)], 8 * H, 1,
                         [(wf if q < 2 else wr)[(q % 2) * hk:] for q in range(4)], Il, 1,
                         [sl[q] for q in range(4)], Il, 1, bf16=bf16)
                dxi = ops.sum_slabs(sl, 4).view(NT, Il)
            return dxi, gwi

        # SIDE_LAG: layer l's side-stream launches are issued (host side) after
        # layer l-1's recurrence launch instead of before it: the GPU runs the
        # same work in the same stream order, but the ~10 launches' host time
        # overlaps that recurrence instead of delaying its launch
        lag = main_first and SIDE_LAG
        pending = None
        for l in range(L - 1, -1, -1):
            inp, h, gates, cell = saved[4 * l:4 * l + 4]
            wf, hf, bif, bhf, wr, hr, bir, bhr = params[8 * l:8 * l + 8]
            l016 = ctx.l016 if l == 0 else None
            dg16 = dgT16 = None     # the bf16 layer-0 operands (l016 only)
            Il = inp.shape[1] if l016 is None else ctx.I
            if l == L - 1 and DEFER_EARLY:
                pre = torch.cuda.Event()      # the decoder backward is done here
                pre.record(main)
            dg = ops.lstm_rec_bwd(dh, gates, cell, hf, hr, H)          # [N,T,8H]
            if l == L - 1:
                # decoder / projection weight gradients, released behind the
                # first BPTT launch (DEFER_EARLY: waiting only for the decoder
                # backward, so they run beside that recurrence too)
                _Deferred.flush(dh.device, after=pre if DEFER_EARLY else None)
            if pending is not None:
                pending()
                pending = None
            dg2 = dg.view(NT, 8 * H)
            if l016 is not None:
                # bf16 operands of the layer-0 data / weight gradients (k-major
                # weight gradient: dg16 serves both, no dg^T copy)
                dg16 = torch.empty(NT, 8 * H, device=dh.device, dtype=torch.bfloat16)
                dgT16 = None if ctx.l016_km else torch.empty(8 * H, NT, device=dh.device,
                                                             dtype=torch.bfloat16)
                ops.cast_bf16_t(dg2, out=dg16, outT=dgT16)
            hp = ops.lstm_hprev(h, H).view(NT, 2 * H)
            ready = torch.cuda.Event()
            ready.record(main)
            side.wait_event(ready)
            # fp32 layer 0: dX and dW_ih in ONE launch on the current stream
            # (gemm_x6r.hip: the weight-gradient tiles first, the data-gradient
            # tiles behind them), instead of dX here beside a split-K weight
            # gradient on the side stream
            pair = (l == 0 and l016 is None and not bf16 and not ops.GEMM_EXACT
                    and (l > 0 or ctx.needs_input_grad[0])
                    and ops.l0_bwd_x6r_eligible(NT, Il, H))
            pair16 = (l == 0 and l016 is not None and not ops.GEMM_EXACT
                      and ctx.needs_input_grad[0] and ops.l0_bwd_bf16_eligible(NT, Il, H))
            # data parallel: the layer-0 input weights' gradients go to the
            # reducer as soon as they exist, bypassing autograd -- after the
            # pair launch (the same kernels as one GPU: its all-reduce then
            # overlaps the whole encoder backward), or chunk by chunk from the
            # side stream where the pair does not run
            to_sink = (l == 0 and ctx.sink is not None and ctx.sink.early_ok
                       and all(p.grad is None for p in ctx.wih0))
            early = to_sink and not (pair or pair16)
            if main_first:
                # the data gradient (the critical path: the next BPTT / the
                # encoder backward wait for it) is issued before the side
                # stream's weight-gradient launches, whose host-side issue
                # would otherwise leave the current stream idle
                dxi, gwi_of[l] = main_dx(l, dg2, inp, Il, wf, wr, l016, pair, to_sink,
                                         dg16, dgT16, pair16)
            def side_work(l=l, dg=dg, dg2=dg2, hp=hp, inp=inp, Il=Il, l016=l016, pair=pair,
                          pair16=pair16, early=early, to_sink=to_sink, dg16=dg16, dgT16=dgT16):
                """Layer l's weight / bias gradients on the side stream (and
                its slots in grads; gwi_of[l] holds the pair's dW_ih)."""
                with torch.cuda.stream(side):
                    # dW_hh = dg^T hprev, dW_ih = dg^T inp: K = N*T rows, tiny outputs
                    # for the recurrent / upper layers -> parallel split-K over row chunks
                    gwh = ops.gemm_tn_splitk(dg2, 8 * H, hp, 2 * H, NT, 4 * H, H,
                                             offsets_b=(0, H), bf16=bf16)
                    if pair or pair16:
                        gwi = None
                    elif early:
                        gwi = _wih_grad_chunked(dg2, inp, H, Il, NT, bf16, ctx.sink, ctx.wih0,
                                                l016=((dg16 if ctx.l016_km else dgT16), l016[0],
                                                      ctx.l016_km) if l016 is not None else None)
                    elif l016 is not None:
                        if ctx.l016_km:
                            gcat = ops.wgrad_bf16_km(dg16, l016[0], NT,
                                                     torch.empty(8 * H, Il, device=dh.device))
                        else:
                            gcat = ops.gemm_bf16nt_splitk(dgT16, l016[0], NT)     # [8H, I]
                        gwi = [gcat[:4 * H], gcat[4 * H:]]
                    else:
                        gwi = ops.gemm_tn_splitk(dg2, 8 * H, inp, Il, NT, 4 * H, Il,
                                                 offsets_b=(0, 0), bf16=bf16)
                    db_ih = ops.colsum(dg2)           # b_ih and b_hh get the same gradient
                    db_hh = db_ih.clone()
                    if dp_side:
                        po = ctx.param_objs[8 * l:8 * l + 8]
                        wi = [None, None] if (early or gwi is None) else gwi
                        _reduce_side(ctx.sink, po, (wi[0], gwh[0], db_ih[:4 * H], db_hh[:4 * H],
                                                    wi[1], gwh[1], db_ih[4 * H:], db_hh[4 * H:]))
                for t in (dg, hp, inp) + ((dg16, dgT16, l016[0]) if l016 is not None else ()):
                    if t is not None:
                        t.record_stream(side)     # main-stream memory read on the side stream
                if pair or pair16:   # (not MAIN_FIRST: set behind main_dx below)
                    gwi = gwi_of.get(l, [None, None])
                if to_sink:   # p.grad set and reduced above / by _wih_grad_chunked
                    gwi = [None, None]
                    ctx.early_done = True
                base = 8 * l
                grads[base + 0], grads[base + 1] = gwi[0], gwh[0]
                grads[base + 2], grads[base + 3] = db_ih[:4 * H], db_hh[:4 * H]
                grads[base + 4], grads[base + 5] = gwi[1], gwh[1]
                grads[base + 6], grads[base + 7] = db_ih[4 * H:], db_hh[4 * H:]

            if lag:
                pending = side_work
            elif main_first:
                side_work()
            else:
                side_work()
                dxi, gwi_of[l] = main_dx(l, dg2, inp, Il, wf, wr, l016, pair, to_sink,
                                         dg16, dgT16, pair16)
                if (pair or pair16) and not to_sink:
                    grads[8 * l], grads[8 * l + 4] = gwi_of[l]
            if l > 0 or ctx.needs_input_grad[0]:
                dh = dxi.view(N, T, Il)
                dx = dh
        if pending is not None:
            pending()
        for gr in grads:
            if gr is not None:
                gr.record_stream(main)    # side-stream memory handed to autograd
        if dp_side or (ctx.sink is None and all(p.grad is None for p in ctx.param_objs)):
            # nothing on the current stream reads these gradients before the
            # optimizer: join the side stream at the end of the backward pass
            # (engine callback) so the layer-0 weight gradient overlaps the
            # encoder backward.  Non-view aliases, so AccumulateGrad stores them
            # instead of cloning (a clone would read them before they exist).
            # Only while every .grad is empty: otherwise AccumulateGrad adds
            # them into .grad on the current stream, which must wait (below).
            dev = dh.device

            torch.autograd.Variable._execution_engine.queue_callback(lambda: _join_side(dev))
            grads = [_alias(gr) if gr is not None else None for gr in grads]
        else:
            # data parallel: the gradient hooks read them as autograd hands them
            # over; accumulation into an existing .grad reads them too
            done = torch.cuda.Event()
            done.record(side)
            main.wait_event(done)
        if ctx.early_done:
            for p in ctx.wih0:            # side-stream .grad buffers read by the optimizer
                p.grad.record_stream(main)
        return (dx, None, None, None, None, None, *grads)


def _wih_grad_chunked(dg2, inp, H, Il, NT, bf16, sink, wih0, rows=None, l016=None):
    """dW_ih_l0 (both directions) on the current (side) stream in gate-row
    chunks of `rows`: dW[r0:r1] = dg[:, r0:r1]^T x, each chunk split-K over
    the N*T reduction into slabs and summed in fixed order straight into the
    parameter's .grad buffer, then handed to the reducer, whose SUM all-reduce
    waits only for that chunk (the 67 MB gradient is produced
    last; its transfer now starts while the remaining chunks, the layer-0
    data gradient and the encoder backward run)."""
    G4 = 4 * H
    rows = H if rows is None else rows       # one gate (i, f, g, o) per chunk
    bufs = [torch.empty(G4, Il, device=dg2.device, dtype=torch.float32) for _ in range(2)]
    if l016 is not None:   # bf16 operands: dg^T [8H, NT], X^T [I, NT] (or k-major dg, X)
        dgT16, XT16, km = l016
        for r0 in range(0, G4, rows):
            for d in range(2):
                chunk = bufs[d][r0:r0 + rows]
                if km:
                    ops.wgrad_bf16_km(dgT16[:, d * G4 + r0:d * G4 + r0 + rows], XT16, NT, chunk)
                else:
                    ops.gemm_bf16nt_splitk(dgT16[d * G4 + r0:d * G4 + r0 + rows], XT16, NT,
                                           out=chunk)
                sink.reduce_chunk(wih0[d], chunk)
        for d in range(2):
            wih0[d].grad = bufs[d]
        return bufs
    tiles = -(-rows // 128) * -(-Il // 128) * 2
    S = ops._chunks_for(NT, tiles)
    kc = NT // S
    slabs = torch.empty(2, S, rows, Il, device=dg2.device, dtype=torch.float32)
    for r0 in range(0, G4, rows):
        ops.gemm(rows, Il, kc, [dg2[:, r0:], dg2[:, G4 + r0:]], 1, 8 * H, [inp, inp], Il, 1,
                 [slabs[0], slabs[1]], Il, 1, strideA=kc * 8 * H, strideB=kc * Il,
                 strideC=rows * Il, nstrided=S, bf16=bf16)
        for d in range(2):
            chunk = bufs[d][r0:r0 + rows]
            ops.sum_slabs(slabs[d], S, out=chunk.view(-1))
            sink.reduce_chunk(wih0[d], chunk)
    for d in range(2):
        wih0[d].grad = bufs[d]
    return bufs


_SIDE_STREAMS: dict = {}   # torch pool streams (never destroyed by torch); cleared at exit
atexit.register(_SIDE_STREAMS.clear)


def _alias(t):
    """A second tensor object on the same storage that is NOT a view: a view
    keeps its base alive, which raises the base's reference count and makes
    autograd's AccumulateGrad clone the gradient instead of stealing it."""
    return torch.empty(0, device=t.device, dtype=t.dtype).set_(
        t.untyped_storage(), t.storage_offset(), t.shape, t.stride())


# release the deferred weight gradients in reverse order (the output
# projection's last, behind the layer-0 pair: C2 16.07 -> 15.96 ms/step,
# profiles/r04kl_summary.txt); AINP_DEFER_LIFO=0: issue order
DEFER_LIFO = os.environ.get("AINP_DEFER_LIFO", "1") != "0"
# the deferred decoder / projection weight gradients wait only for the decoder
# backward (an event recorded before the first BPTT launch), not for that
# recurrence as well, so they run beside it on the CUs it leaves idle
# (AINP_DEFER_EARLY=0: behind it; C2 14.54 -> 13.89, C3-shape 8.55 -> 8.39
# ms/step on one box, profiles/r05i_ab_defer_early.txt).  A CU-masked side
# stream (hipExtStreamCreateWithCUMask, 8 of 32 CUs kept free for the
# recurrence) measured +3.3 ms/step on both and was dropped.
DEFER_EARLY = os.environ.get("AINP_DEFER_EARLY", "1") != "0"
# BLSTM backward: each layer's side-stream weight-gradient launches issued
# behind the next layer's recurrence launch (_BLSTMFn.backward; A/B:
# AINP_SIDE_LAG=0)
SIDE_LAG = os.environ.get("AINP_SIDE_LAG", "1") != "0"
# (C2 14.65 -> 14.43 / 14.79 -> 14.55 ms/step A/B, profiles/r05o_ab_x6r_apf_side2.txt).
# Round 6: AINP_BLSTM_SIDE2 = 0 / 1 / fp32 (default) / bf16 -- in the bf16
# configuration the second stream's GEMMs slowed the layer-0 BPTT beside them
# (0.31 -> up to 0.48 ms) more than queueing them behind the deferred work
# costs: C3 6.89 / 6.91 -> 6.86 / 6.81 and, on a second box, 6.88 / 6.82 ->
# 6.76 / 6.74 ms/step; C2 13.53 -> 14.02 without it (profiles/r06_ab_blstm_side2.txt)
BLSTM_SIDE2 = os.environ.get("AINP_BLSTM_SIDE2", "fp32")


def _blstm_side2(bf16):
    return BLSTM_SIDE2 == "1" or BLSTM_SIDE2 == ("bf16" if bf16 else "fp32")


# Round 6: AINP_ENC_SIDE2 = 0 / 1 / fp32 / bf16: in which configurations the
# encoder's inner weight gradients use the second side stream (idle by then),
# so the 16 -> 32 one starts behind its own data gradient instead of behind
# the 32 -> 64 one, which ends the C2 backward (profiles/r06m_ab_enc_side2.txt:
# C2 14.82 / 14.86 -> 14.70 / 14.79 ms/step, C3 mixed +-0.06: fp32 only)
ENC_SIDE2 = os.environ.get("AINP_ENC_SIDE2", "fp32")


def _enc_side2(bf16):
    return ENC_SIDE2 == "1" or ENC_SIDE2 == ("bf16" if bf16 else "fp32")


class _Deferred:
    """Weight-gradient launches queued during the backward (decoder convs,
    projection) and released onto the side stream at a chosen point -- when
    the first BPTT recurrence has been launched -- so they fill the CUs that
    latency-bound kernel leaves idle instead of competing with the decoder's
    data-gradient chain.  Their output tensors are handed to autograd at
    queue time (written later); an engine callback releases anything left and
    makes the current stream join the side stream before the backward ends."""

    _queues: dict = {}

    @classmethod
    def push(cls, device, fn, inputs, outputs, params=(), sink=None, first=False):
        """params / sink (data parallel): the Parameters the outputs are the
        gradients of, and the GradAllReducer that all-reduces them from the side
        stream once they are written (its hooks skip them meanwhile).
        first: released ahead of the others (a short job that must not be
        left to run starved beside the layer-0 GEMM pair)."""
        q = cls._queues.setdefault(device, [])
        if not q:
            torch.autograd.Variable._execution_engine.queue_callback(
                lambda: cls.flush(device, join=True))
        if sink is not None and sink.early_ok:
            for p in params:
                sink.defer(p)
        else:
            sink = None
        q.append((fn, inputs, outputs, params, sink, first))

    @classmethod
    def flush(cls, device, join=False, after=None):
        """after: an event recorded earlier on the current stream for the side
        stream to wait on instead of everything issued so far."""
        q = cls._queues.pop(device, [])
        if DEFER_LIFO:
            # last queued first: the output projection's weight gradient (a
            # short full-width GEMM) ahead of the decoder convs' (persistent
            # kernels), so it does not run starved beside the layer-0 pair
            q = q[::-1]
        # the short 1-channel-side weight gradients first: behind the others
        # they met the layer-0 GEMM pair, whose 160 KB / full-VGPR workgroups
        # leave no room on a CU (16 -> 1: 1.6 ms there against 0.05 ms)
        q = [j for j in q if j[5]] + [j for j in q if not j[5]]
        if q:
            with _side_work(device, callback=False, after=after) as sw:
                for fn, inputs, outputs, params, sink, _first in q:
                    fn()
                    sw.handoff(inputs, outputs)
                    if sink is not None:
                        for p, o in zip(params, outputs):
                            sink.reduce_chunk(p, o, kind="side")
        if join and q is not None:
            _join_side(device)


def _reduce_side(sink, params, grads):
    """Data parallel: hand side-stream gradients to the reducer from the side
    stream (call inside its context): the all-reduce waits for that stream's
    work, not for the compute stream; the reducer's hooks skip them."""
    if sink is None or not sink.early_ok:
        return False
    for p, g in zip(params, grads):
        if p is not None and g is not None:
            sink.defer(p)
            sink.reduce_chunk(p, g, kind="side")
    return True


class _side_work:
    """Context: queue work on the device's side stream after everything the
    current stream has issued so far; the current stream joins the side stream
    at the end of the backward pass (autograd engine callback), before any
    optimizer step can read what the side stream produced."""

    def __init__(self, device, callback=True, after=None, k=0):
        self.device = device
        self.callback = callback
        self.after = after
        self.k = k

    def __enter__(self):
        dev = self.device
        self.main = torch.cuda.current_stream(dev)
        self.side = _side_stream(dev, self.k)
        ev = self.after
        if ev is None:
            ev = torch.cuda.Event()
            ev.record(self.main)
        self.side.wait_event(ev)
        self._ctx = torch.cuda.stream(self.side)
        self._ctx.__enter__()

        if self.callback:
            torch.autograd.Variable._execution_engine.queue_callback(lambda: _join_side(dev))
        return self

    def handoff(self, inputs, outputs):
        """Caching-allocator bookkeeping: inputs (made on the current stream)
        are read on the side stream; outputs (made on the side stream) are
        read later on the current one."""
        for t in inputs:
            t.record_stream(self.side)
        for t in outputs:
            if t is not None:
                t.record_stream(self.main)

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        return False


def _side_stream(device, k=0):
    """Side stream k of the device (0: deferred conv / projection weight
    gradients; 1: the BLSTM's weight gradients under BLSTM_SIDE2)."""
    s = _SIDE_STREAMS.get((device, k))
    if s is None:
        s = torch.cuda.Stream(device=device)
        _SIDE_STREAMS[(device, k)] = s
    return s


def _join_side(device):
    """The current stream waits for everything issued so far on the device's
    side streams."""
    cur = torch.cuda.current_stream(device)
    for (d, _k), s in list(_SIDE_STREAMS.items()):
        if d == device:
            ev = torch.cuda.Event()
            ev.record(s)
            cur.wait_event(ev)


# ------------------------------------------------------------------ projection
class _ProjFn(torch.autograd.Function):
    """nn.Linear(2H, C*F) + view(N,T,C,F).permute(0,2,3,1) -> [N, C, F, T]."""

    @staticmethod
    def forward(ctx, h, w, b, C, F, bf16=False, defer_wgrad=False, sink=None):
        N, T, K = h.shape
        out = torch.empty(N, C, F, T, device=h.device, dtype=torch.float32)
        NO = C * F
        # per example n: out_n[t][col] = h_n[t] . w[col] + b[col], stored col*T + t
        ops.gemm(T, NO, K, [h], K, 1, [w], 1, K, [out], 1, T, strideA=T * K,
                 strideC=NO * T, nstrided=N, bias1=[b], bf16=bf16)
        ctx.save_for_backward(h, w)
        ctx.shape = (N, C, F, T)
        ctx.bf16 = bf16
        ctx.defer_wgrad = defer_wgrad
        ctx.sink = sink
        ctx.param_objs = (w, b)
        # the consumer's data gradient may hand back [C, F, N, T] storage (see
        # _ConvStackFn.backward, AINP_PROJ_CFNT=0: NCHW and the copy below)
        out._ainp_cfnt_grad = PROJ_CFNT and _ProjFn._x6(bf16, N * T, NO, K)
        return out

    @staticmethod
    def backward(ctx, g):
        h, w = ctx.saved_tensors
        N, C, F, T = ctx.shape
        NO = C * F
        K = h.shape[2]
        if _ProjFn._x6(ctx.bf16, N * T, NO, K):
            return _ProjFn._backward_x6(ctx, g, h, w)
        g = g.contiguous()
        # dh_n[t][k] = sum_col g_n[col][t] w[col][k]: only 6 output tiles per
        # example, so the col sum (K = C*F) is split over S pointer batches into
        # slabs (4x the workgroups) and combined in fixed order
        S = 4 if NO % 4 == 0 else 1
        kc = NO // S
        hs = torch.empty(S, N, T, K, device=h.device, dtype=torch.float32)
        gflat = g.view(-1)
        ops.gemm(T, K, kc, [gflat[s * kc * T:] for s in range(S)], 1, T,
                 [w[s * kc:] for s in range(S)], K, 1, [hs[s] for s in range(S)], K, 1,
                 strideA=NO * T, strideC=T * K, nstrided=N, bf16=ctx.bf16)
        dh = hs[0] if S == 1 else ops.sum_slabs(hs, S).view(N, T, K)
        # dw[col][k] = sum_{n,t} g_n[col][t] h_n[t][k]: split the example sum
        # over S pointer batches (S partial slabs, ksplit mode 2) so the small
        # [C*F, 2H] output still fills the chip, then combine in fixed order.
        bf16 = ctx.bf16

        def wgrad(dw, db, g=g, h=h):
            S = ops.split_count(N)
            per = N // S
            slabs = torch.empty(S, NO, K, device=h.device, dtype=torch.float32)
            ops.gemm(NO, K, T, [g[i * per] for i in range(S)], T, 1,
                     [h[i * per] for i in range(S)], K, 1, [slabs[i] for i in range(S)], K, 1,
                     strideA=NO * T, strideB=T * K, nstrided=per, ksplit=2, bf16=bf16)
            ops.sum_slabs(slabs, S, out=dw.view(-1))
            # db[col] = sum_{n,t} g_n[col][t]
            ops.rowsum_batched(g.view(N, NO, T), out=db)
        dw = torch.empty(NO, K, device=g.device)
        db = torch.empty(NO, device=g.device)
        if ctx.defer_wgrad:
            dwv, dbv = _alias(dw), _alias(db)     # aliases only (see _ConvStackFn)
            _Deferred.push(g.device, lambda: wgrad(dwv, dbv), (g, h), (dwv, dbv),
                           params=ctx.param_objs, sink=ctx.sink)
        else:
            wgrad(dw, db)
        return dh, dw, db, None, None, None, None, None

    @staticmethod
    def _x6(bf16, NT, NO, K):
        return not bf16 and not ops.GEMM_EXACT and ops.proj_bwd_x6_eligible(NT, NO, K)

    @staticmethod
    def _backward_x6(ctx, g, h, w):
        """fp32: both gradients on the x6r MFMA tile (ops.proj_bwd_x6) from the
        gradient permuted once to [C*F, N*T] -- every column of the reduction
        then lies at one stride, where the [N][C*F][T] layout needs a pointer
        batch per example."""
        N, C, F, T = ctx.shape
        NO, K = C * F, h.shape[2]
        gq = g.permute(1, 2, 0, 3)
        if gq.is_contiguous():   # [C, F, N, T] storage (the decoder's dgrad wrote it)
            gp = gq.view(NO, N * T)
        else:
            gp = g.contiguous().view(N, NO, T).transpose(0, 1).contiguous().view(NO, N * T)
        h2 = h.view(N * T, K)
        dh = torch.empty(N, T, K, device=g.device, dtype=torch.float32)
        dw = torch.empty(NO, K, device=g.device)
        db = torch.empty(NO, device=g.device)
        if ctx.defer_wgrad:
            ops.proj_bwd_x6(gp, h2, w, dh=dh.view(N * T, K))

            def wgrad(dw, db):
                ops.proj_bwd_x6(gp, h2, w, dw=dw)
                ops.rowsum_batched(gp.view(1, NO, N * T), out=db)
            dwv, dbv = _alias(dw), _alias(db)
            _Deferred.push(g.device, lambda: wgrad(dwv, dbv), (gp, h), (dwv, dbv),
                           params=ctx.param_objs, sink=ctx.sink)
        else:
            ops.proj_bwd_x6(gp, h2, w, dh=dh.view(N * T, K), dw=dw)
            ops.rowsum_batched(gp.view(1, NO, N * T), out=db)
        return dh, dw, db, None, None, None, None, None


# ------------------------------------------------------------------ loss
class _L1Pow10LossFn(torch.autograd.Function):
    """nn.L1Loss(reduction='sum')((10 ** y) * m, |target| * m)."""

    @staticmethod
    def forward(ctx, y, mask, target):
        y = y.contiguous()
        loss, dy = ops.l1_pow10_loss(y, mask.contiguous(), target.contiguous(),
                                     want_grad=y.requires_grad)
        ctx.save_for_backward(dy if dy is not None else y)
        return loss.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return ops.scale_by_scalar(dy, g), None, None


def l1_pow10_loss(y, mask, target):
    """Training loss of models/CNNBLSTM/train.py:104 on the fused kernel."""
    return _L1Pow10LossFn.apply(y, mask, target)


train_step_reference_loss = l1_pow10_loss


# ------------------------------------------------------------------ module
class StackedBLSTMCNN(nn.Module):
    """Drop-in for models/CNNBLSTM/model.py:StackedBLSTMCNN."""

    def __init__(self, config_path=None, config: dict | None = None):
        super().__init__()
        full_cfg = config if config is not None else load_config(config_path)
        mdl_cfg = full_cfg["model"]
        self.in_channels = mdl_cfg["in_channels"]
        self.n_layers = mdl_cfg["num_lstm_layers"]
        self.hidden_dim = mdl_cfg["lstm_hidden_dim"]
        self.freq_bins = full_cfg["data"]["spectrogram"]["n_fft"] // 2 + 1
        self.using_phase = self.in_channels == 2
        self.enc_filters = mdl_cfg["enc_filters"]
        self.dec_filters = mdl_cfg["dec_filters"]
        # optional accel block (not in the reference YAML): compute precision of
        # the GEMMs / 16-64 channel convs; "bf16" = bf16 operands, fp32 accumulate,
        # fp32 LSTM cell state, BatchNorm statistics and master weights (C3)
        dtype = (full_cfg.get("accel") or {}).get("dtype", "fp32")
        if dtype not in ("fp32", "bf16"):
            raise ValueError(f"accel.dtype must be fp32 or bf16, got {dtype!r}")
        self.bf16 = dtype == "bf16"
        # accel.deterministic (default true): every kernel on the path reduces in
        # a fixed order, so runs are bit-reproducible; true also makes the one
        # atomic-accumulating entry point (ops.colsum(accumulate=True)) raise
        det = (full_cfg.get("accel") or {}).get("deterministic", True)
        if not isinstance(det, bool):
            raise ValueError(f"accel.deterministic must be true or false, got {det!r}")
        self.deterministic = det
        ops.set_deterministic(det)
        # identical construction order to model.py:34-61 (same init RNG draws)
        self.encoder = nn.Sequential(
            nn.Conv2d(self.in_channels, self.enc_filters[0], kernel_size=3, padding=1),
            nn.BatchNorm2d(self.enc_filters[0]),
            nn.ReLU(),
            nn.Conv2d(self.enc_filters[0], self.enc_filters[1], kernel_size=3, padding=1),
            nn.BatchNorm2d(self.enc_filters[1]),
            nn.ReLU(),
            nn.Conv2d(self.enc_filters[1], self.hidden_dim // 2, kernel_size=3, padding=1),
            nn.BatchNorm2d(self.hidden_dim // 2),
            nn.ReLU(),
        )
        self.lstm = nn.LSTM(input_size=self.freq_bins * self.hidden_dim // 2,
                            hidden_size=self.hidden_dim, num_layers=self.n_layers,
                            batch_first=True, bidirectional=True)
        self.projection = nn.Linear(self.hidden_dim * 2, self.freq_bins * self.dec_filters[0])
        self.decoder = nn.Sequential(
            nn.Conv2d(self.dec_filters[0], self.dec_filters[1], kernel_size=3, padding=1),
            nn.BatchNorm2d(self.dec_filters[1]),
            nn.ReLU(),
            nn.Conv2d(self.dec_filters[1], self.dec_filters[0], kernel_size=3, padding=1),
            nn.BatchNorm2d(self.dec_filters[0]),
            nn.ReLU(),
            nn.Conv2d(self.dec_filters[0], self.in_channels, kernel_size=3, padding=1),
        )
        self.comm = None  # set by ainp.dist for SyncBN across DP ranks
        # set to an ainp.dist.GradAllReducer (data parallel): the layer-0 input
        # weight gradients are computed in chunks and all-reduced as they complete
        self.grad_reducer = None
        # decoder / projection weight gradients overlap the BPTT on a side stream
        self.defer_wgrad = os.environ.get("AINP_DEFER_WGRAD", "1") != "0"
        self.defer_wgrad_encoder = os.environ.get("AINP_DEFER_ENC", "1") != "0"

    # -- helpers ----------------------------------------------------------
    @staticmethod
    def _stack(seq):
        spec, params = [], []
        mods = list(seq)
        i = 0
        while i < len(mods):
            conv = mods[i]
            bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) else None
            params += [conv.weight, conv.bias]
            if bn is not None:
                params += [bn.weight, bn.bias]
                spec.append((True, bn))
                i += 3  # conv, bn, relu
            else:
                spec.append((False, None))
                i += 1
        return spec, params

    def forward(self, x):
        """x: (batch, in_channels, freq_bins, timeframes) -> (batch, F, T)."""
        if x.device.type != "cuda":
            raise RuntimeError("ainp StackedBLSTMCNN runs on the MI355X kernels only; "
                               "move the model and inputs to a GPU")
        batch_size, _, freq_bins, timeframes = x.shape
        x = x.contiguous()
        spec, params = self._stack(self.encoder)
        # layer-0 bf16 operands (encoder -> BLSTM)
        box = {"H": self.hidden_dim} if self.bf16 else None
        # the deferred weight gradients are written after autograd receives
        # them: only while the .grad buffers are empty (nothing accumulates)
        sink = self.grad_reducer if (self.training and torch.is_grad_enabled()) else None
        if sink is not None:    # BLSTM side-stream reductions follow the same switch
            sink.side_ok = self.defer_wgrad
        # data parallel keeps these overlaps: the deferred gradients are
        # all-reduced from the side stream once written (_reduce_side)
        defer_enc = (self.defer_wgrad_encoder and self.training and torch.is_grad_enabled()
                     and all(q.grad is None for q in self.encoder.parameters()))
        z = _ConvStackFn.apply(x, spec, self.training, True, self.comm, self.bf16, box,
                               (defer_enc, sink), *params)
        z = _BLSTMFn.apply(z, self.hidden_dim, self.n_layers, self.bf16, sink, box,
                           *self.lstm._flat_weights)
        # decoder / projection weight gradients on the side stream, overlapping the
        # BPTT recurrence (64 workgroups); only while the .grad buffers are empty
        # (the deferred outputs are written after autograd receives them, so
        # they cannot be accumulated into); under data parallelism they are
        # all-reduced from the side stream when written
        defer = (self.defer_wgrad and self.training and torch.is_grad_enabled()
                 and all(q.grad is None for m in (self.projection, self.decoder)
                         for q in m.parameters()))
        # model.py:82 hard-codes 16 decoder channels
        p = _ProjFn.apply(z, self.projection.weight, self.projection.bias, 16, freq_bins,
                          self.bf16, defer, sink)
        spec, params = self._stack(self.decoder)
        y = _ConvStackFn.apply(p, spec, self.training, False, self.comm, self.bf16, None,
                               ("queue" if defer else False, sink), *params)
        return y.squeeze(1)

    def reconstruct_spectrogram(self, log_spectrogram_gap, gap_mask):
        """model.py:92-108: model output inside the gap, input elsewhere."""
        if not self.using_phase:
            rec = self(log_spectrogram_gap.unsqueeze(1))
        else:
            rec = self(log_spectrogram_gap)
        gap_mask = gap_mask.float()
        if self.using_phase:
            rec = rec[:, 0, :, :] + rec[:, 1, :, :] * 1j
            log_spectrogram_gap = log_spectrogram_gap[:, 0, :, :] + log_spectrogram_gap[:, 1, :, :] * 1j
        return rec * gap_mask + log_spectrogram_gap * (1 - gap_mask)
