"""torch.autograd wrappers over the C ABI (``include/a3vt.h``).  PyTorch is plumbing here: it owns device
memory, the current HIP stream and autograd bookkeeping; every op below is one C call into ``liba3vt.so``.

All tensors must be float32 / int32, contiguous, on a ROCm device.  There is no CPU path.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import lib as _lib
from .mesh import CSRAdjacency


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"a3vt: `{name}` must be a tensor on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"a3vt: `{name}` must be {dtype}, got {t.dtype}")
    return t.contiguous()


_WORKSPACES = {}
# call counters (tests assert that forward-only callers never allocate the activation stash)
STATS = {"stack_calls": 0, "stack_stash_calls": 0}


def workspace(tag, nbytes, device):
    """Per-device scratch buffer that only grows; all users run on the current stream, in order."""
    key = (tag, device.index if device.index is not None else torch.cuda.current_device())
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4 + 64, dtype=torch.float32, device=device)
        _WORKSPACES[key] = buf
    return buf


class DeviceCSR:
    """Row-normalised adjacency (and its transpose) as int32/float32 device tensors."""

    def __init__(self, host: CSRAdjacency, device):
        self.n, self.nnz = host.n, host.nnz
        L = _lib.load()
        _lib.check(L.a3vt_csr_validate(host.rowptr.ctypes.data, host.col.ctypes.data, host.n, host.nnz), "csr_validate")
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        self.rowptr, self.col, self.val = to(host.rowptr), to(host.col), to(host.val)
        self.t_rowptr, self.t_col, self.t_val = to(host.t_rowptr), to(host.t_col), to(host.t_val)
        self.host = host
        self.max_degree = int(np.diff(host.rowptr).max()) if host.n else 0        # hub rows get their own launch
        self.t_max_degree = int(np.diff(host.t_rowptr).max()) if host.n else 0
        # the fused vision + touch matrix as P + a complete bipartite block (a3vt_adj_split): found on the host, PROVEN
        # against the CSR by the library, handed to the stack calls next to the CSR.  Plain meshes keep split = None
        # (their rows are short already: the generic kernels serve them bit for bit as before).
        self.split = self.split_struct = None
        sp = host.split() if self.max_degree > 8 else None
        if sp is not None:
            _lib.check(L.a3vt_adj_split_validate(host.rowptr.ctypes.data, host.col.ctypes.data, host.val.ctypes.data, host.n,
                                                 sp.rowptr.ctypes.data, sp.col.ctypes.data, sp.scale.ctypes.data,
                                                 sp.cls.ctypes.data), "adj_split_validate")
            self.split = (to(sp.rowptr), to(sp.col), to(sp.scale), to(sp.cls))
            self.split_struct = _lib.AdjSplit(*[t.data_ptr() for t in self.split], sp.max_degree, sp.n_seam, sp.n_centre)
        self.use_split = True     # test hook: False = the plain CSR everywhere (A/B of the two aggregations)

    def split_ref(self):
        """``const a3vt_adj_split *`` for a stack call (NULL without a split)."""
        return ctypes.byref(self.split_struct) if (self.split_struct is not None and self.use_split) else None

    @property
    def device(self):
        return self.val.device


def _wants_grad(*tensors):
    """Whether a backward pass can follow this call.  Decided OUTSIDE ``Function.forward``: inside it
    ``ctx.needs_input_grad`` is still True for parameters under ``torch.no_grad()`` (it mirrors ``requires_grad``, not the
    grad mode), which would make the forward-only callers (``Engine.validate``, ``policies/scoring.py``) allocate and write
    the whole activation stash."""
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


GEMM_MODES = {"fp32": 0, "bf16": 1, "bf16s": 2, "fp32x3": 3}


PATH_NAMES = ("stack_quad", "stack_rows", "rowgemm_adirect", "rowgemm3", "dw3", "dw_hybrid", "rowgemm16", "stack16_quad", "rowgemm_w", "dw_w", "stack_split", "csr16_tiles",
              "qnet_input_fwd", "qnet_input_bwd", "fold_fwd", "fold_bwd", "csr3_split")


def path_counts(reset=False):
    """Launch decisions per kernel family since the last reset (``a3vt_dbg_path_counts``): a test hook — parity tests assert
    that their fixture reaches the kernels it claims to pin."""
    import ctypes
    buf = (ctypes.c_longlong * len(PATH_NAMES))()
    _lib.load().a3vt_dbg_path_counts(buf, len(PATH_NAMES), 1 if reset else 0)
    return dict(zip(PATH_NAMES, (int(x) for x in buf)))


def _launch_counts(symbol, names, reset):
    """One ``a3vt_*_launches(counts, reset)`` hook read into ``{name: count}``."""
    buf = (ctypes.c_longlong * len(names))()
    getattr(_lib.load(), symbol)(buf, 1 if reset else 0)
    return dict(zip(names, (int(x) for x in buf)))


def nn_work(enable):
    """Work counters of the pruned nearest-neighbour search (``a3vt_dbg_nn_work``; a test hook, synchronises the device):
    returns what was counted since they were switched on, then switches them on (True: cleared first) or off (False)."""
    import ctypes
    buf = (ctypes.c_ulonglong * 8)()
    _lib.check(_lib.load().a3vt_dbg_nn_work(1 if enable else 0, buf), "dbg_nn_work")
    names = ("waves", "groups", "blocks", "box_tests", "max_groups_per_wave")
    return dict(zip(names, (int(x) for x in buf)))


def gemm_mode(bf16):
    """0 exact fp32 MFMA; 1 bf16 operands, fp32 storage; 2 bf16 storage (activations / gradients / weight images bf16 in
    HBM, fp32 accumulation); 3 "fp32x3": fp32 storage, the hidden-layer products as six bf16 MFMA passes on operands split
    exactly into three bf16 pieces (fp32-level error, not bit-identical to mode 0; csrc/gcn_gemm3.hip).  Accepts the mode
    number, a bool (True = 1) or the ``args.gemm_precision`` string."""
    if isinstance(bf16, str):
        return GEMM_MODES[bf16]
    return int(bf16)


class GradSink:
    """Where the gradient of one parameter lives (a view into a trainer's flat all-reduce bucket,
    ``distributed.FlatGradBucket``).  Library calls that produce parameter gradients write them there directly — the first
    use of a step overwrites, later uses (``mesh_deform_2`` serves stages 2 and 3) accumulate inside the kernel — instead of
    returning fresh tensors for autograd to assign, add up and the bucket to copy.  ``expect`` counts the forward uses of the
    step whose backward has not run yet; ``on_final`` fires when it returns to zero (the gradient is complete)."""
    __slots__ = ("view", "written", "expect", "on_final")

    def __init__(self, view, on_final=None):
        self.view, self.written, self.expect, self.on_final = view, False, 0, on_final

    def reset(self):
        self.written, self.expect = False, 0


GRAD_SINKS = {}     # id(parameter) -> (weakref to the parameter, GradSink); filled by FlatGradBucket, consulted by GCNStackFn


def register_grad_sink(param, view, on_final=None):
    sink = GradSink(view, on_final)
    key = id(param)
    # the weak reference both proves identity at lookup time (ids are reused once a Parameter is freed) and drops the
    # entry — and with it the reference to the owner's flat buffer — when the parameter dies
    def _gone(ref, key=key):
        if GRAD_SINKS.get(key, (None,))[0] is ref:
            del GRAD_SINKS[key]

    GRAD_SINKS[key] = (weakref.ref(param, _gone), sink)
    return sink


def unregister_grad_sink(param, sink=None):
    """Remove ``param``'s sink (only if it is ``sink``, when given: a newer bucket may have registered its own since)."""
    ent = GRAD_SINKS.get(id(param))
    if ent is not None and ent[0]() is param and (sink is None or ent[1] is sink):
        del GRAD_SINKS[id(param)]


def grad_sink_of(param):
    """The sink registered for exactly this parameter object, or None."""
    ent = GRAD_SINKS.get(id(param))
    return ent[1] if ent is not None and ent[0]() is param else None


class GCNStackFn(torch.autograd.Function):
    """One GCN (reference ``GCN.forward``, vision/model.py:316-331): feats (B,N,ld) -> update (B,N,3)."""

    @staticmethod
    def forward(ctx, feats, adj, in_features, hidden, cut_len, bf16, need_bwd, *params):
        L = _lib.load()
        feats = _req(feats, "feats")
        B, N, ld = feats.shape
        if N != adj.n:
            raise RuntimeError(f"a3vt: features have {N} vertices but the adjacency has {adj.n}")
        weights = [_req(p, "weight") for p in params[0::2]]
        biases = [_req(p, "bias") for p in params[1::2]]
        nl = len(weights)
        mode = gemm_mode(bf16)
        acts = masks = None
        STATS["stack_calls"] += 1
        if need_bwd and nl > 1:
            STATS["stack_stash_calls"] += 1
            ab, mb = ctypes.c_size_t(0), ctypes.c_size_t(0)
            _lib.check(L.a3vt_gcn_stack_stash_bytes(B, N, hidden, nl, cut_len, mode, ctypes.byref(ab), ctypes.byref(mb)),
                       "gcn_stack_stash_bytes")
            acts = torch.empty(ab.value, dtype=torch.uint8, device=feats.device)    # fp32 or bf16 rows, by mode
            masks = torch.empty(mb.value, dtype=torch.uint8, device=feats.device)
        nbytes = L.a3vt_gcn_stack_scratch_bytes_mode(B, N, in_features, hidden, nl, cut_len, 1 if need_bwd else 0, mode)
        scratch = workspace("gcn", nbytes, feats.device)
        update = torch.empty((B, N, 3), dtype=torch.float32, device=feats.device)
        wp, bp = _ptr_array(weights), _ptr_array(biases)
        _lib.check(L.a3vt_gcn_stack_fwd_adj(_lib.ptr(feats), ld, in_features, wp, bp, nl, hidden, cut_len,
                                            _lib.ptr(adj.rowptr), _lib.ptr(adj.col), _lib.ptr(adj.val),
                                            max(adj.max_degree, adj.t_max_degree), adj.split_ref(), N, B, mode,
                                            _lib.ptr(acts), _lib.ptr(masks), _lib.ptr(scratch), _lib.ptr(update), _stream()),
                   "gcn_stack_fwd")
        ctx.adj, ctx.dims, ctx.mode = adj, (in_features, hidden, cut_len, nl), mode
        ctx.acts, ctx.masks = acts, masks
        # gradients written where they live: every parameter of this call has a sink in the trainer's flat bucket
        sinks = [grad_sink_of(p) for p in params] if need_bwd else []
        ctx.sinks = sinks if sinks and all(k is not None and k.view.shape == p.shape and k.view.is_contiguous()
                                           for k, p in zip(sinks, params)) else None
        if ctx.sinks:
            for k in ctx.sinks:
                k.expect += 1
        ctx.save_for_backward(feats, *weights, *biases)
        return update

    @staticmethod
    def backward(ctx, grad_update):
        L = _lib.load()
        in_features, hidden, cut_len, nl = ctx.dims
        feats = ctx.saved_tensors[0]
        weights = list(ctx.saved_tensors[1:1 + nl])
        biases = list(ctx.saved_tensors[1 + nl:1 + 2 * nl])
        adj = ctx.adj
        B, N, ld = feats.shape
        grad_update = _req(grad_update, "grad_update")
        sinks = ctx.sinks
        if sinks and len({k.written for k in sinks}) != 1:     # mixed first / later uses: take the ordinary path
            for k in sinks:
                k.expect -= 1
            sinks = None
        if sinks:
            acc = 1 if sinks[0].written else 0
            gw = [k.view for k in sinks[0::2]]
            gb = [k.view for k in sinks[1::2]]
        else:
            acc = 0
            gw = [torch.empty_like(w) for w in weights]
            gb = [torch.empty_like(b) for b in biases]
        gfeats = torch.empty_like(feats)
        nbytes = L.a3vt_gcn_stack_scratch_bytes_mode(B, N, in_features, hidden, nl, cut_len, 1, ctx.mode)
        scratch = workspace("gcn", nbytes, feats.device)
        _lib.check(L.a3vt_gcn_stack_bwd_adj(_lib.ptr(feats), ld, in_features, _ptr_array(weights), _ptr_array(biases), nl,
                                            hidden, cut_len, _lib.ptr(adj.rowptr), _lib.ptr(adj.col), _lib.ptr(adj.val),
                                            _lib.ptr(adj.t_rowptr), _lib.ptr(adj.t_col), _lib.ptr(adj.t_val),
                                            max(adj.max_degree, adj.t_max_degree), adj.split_ref(), N, B, ctx.mode,
                                            _lib.ptr(ctx.acts), _lib.ptr(ctx.masks), _lib.ptr(grad_update), _ptr_array(gw),
                                            _ptr_array(gb),
                                            _lib.ptr(gfeats), _lib.ptr(scratch), acc, _stream()), "gcn_stack_bwd")
        ctx.acts = ctx.masks = None
        if sinks:   # the gradients are in the bucket already: nothing for autograd to assign or add
            for k in sinks:
                k.written = True
                k.expect -= 1
            for k in sinks:
                if k.expect == 0 and k.on_final is not None:
                    k.on_final()
            return (gfeats, None, None, None, None, None, None, *([None] * (2 * nl)))
        grads = []
        for w, b in zip(gw, gb):
            grads += [w, b]
        return (gfeats, None, None, None, None, None, None, *grads)


def gcn_stack(feats, adj, in_features, hidden, cut_len, weights, biases, bf16=False):
    """``bf16``: gemm mode of the per-vertex products (:func:`gemm_mode`): False / 0 = exact fp32 (default, the parity
    mode); True / 1 / "bf16" = operands rounded to bf16 on their way into the matrix pipe; 2 / "bf16s" = bf16 storage of
    activations and gradients as well (BASELINE configs[3]/[4])."""
    params = []
    for w, b in zip(weights, biases):
        params += [w, b]
    return GCNStackFn.apply(feats, adj, in_features, hidden, cut_len, gemm_mode(bf16), _wants_grad(feats, *params), *params)


class GCNLayerFn(torch.autograd.Function):
    """One GCN layer (reference ``GCN_layer.forward``, vision/model.py:351-363) for callers with their own layer loop:
    x (B,N,ld) -> y (B,N,out).  ``cut_len`` = out for a layer without the cut."""

    @staticmethod
    def forward(ctx, x, adj, weight, bias, cut_len, relu, bf16=False, need_bwd=True):
        L = _lib.load()
        x = _req(x, "features")
        weight, bias = _req(weight, "weight"), _req(bias, "bias")
        B, N, ld = x.shape
        if N != adj.n:
            raise RuntimeError(f"a3vt: features have {N} vertices but the adjacency has {adj.n}")
        kin, nout = weight.shape[-2], weight.shape[-1]
        if ld % 4 != 0 or ld < kin:
            raise RuntimeError(f"a3vt: feature row length {ld} must be a multiple of 4 and >= in_features={kin}")
        ldy = (nout + 3) // 4 * 4
        y = torch.empty((B, N, ldy), dtype=torch.float32, device=x.device)
        scratch = workspace("gcn", L.a3vt_gcn_layer_scratch_bytes(B, N, ld, nout, cut_len, 1 if need_bwd else 0),
                            x.device)
        _lib.check(L.a3vt_gcn_layer_fwd(_lib.ptr(x), ld, kin, _lib.ptr(weight), _lib.ptr(bias), nout, cut_len,
                                        1 if relu else 0, _lib.ptr(adj.rowptr), _lib.ptr(adj.col), _lib.ptr(adj.val),
                                        adj.max_degree, N, B, 1 if bf16 else 0, _lib.ptr(y), ldy, _lib.ptr(scratch),
                                        _stream()), "gcn_layer_fwd")
        ctx.adj, ctx.dims, ctx.bf16 = adj, (kin, nout, cut_len, bool(relu), ldy), bool(bf16)
        ctx.save_for_backward(x, weight, y)
        return y[..., :nout] if ldy != nout else y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.load()
        kin, nout, cut_len, relu, ldy = ctx.dims
        x, weight, y = ctx.saved_tensors
        adj = ctx.adj
        B, N, ld = x.shape
        gy = _req(gy, "grad_output")
        gw, gb, gx = torch.empty_like(weight), torch.empty(nout, dtype=torch.float32, device=x.device), torch.empty_like(x)
        scratch = workspace("gcn", L.a3vt_gcn_layer_scratch_bytes(B, N, ld, nout, cut_len, 1), x.device)
        _lib.check(L.a3vt_gcn_layer_bwd(_lib.ptr(x), ld, kin, _lib.ptr(weight), nout, cut_len, 1 if relu else 0,
                                        _lib.ptr(adj.t_rowptr), _lib.ptr(adj.t_col), _lib.ptr(adj.t_val),
                                        adj.t_max_degree, N, B, 1 if ctx.bf16 else 0,
                                        _lib.ptr(y), ldy, _lib.ptr(gy), gy.shape[-1], _lib.ptr(gw), _lib.ptr(gb),
                                        _lib.ptr(gx), _lib.ptr(scratch), _stream()), "gcn_layer_bwd")
        return gx, None, gw, gb, None, None, None, None


def gcn_layer(x, adj, weight, bias, cut_len, relu, bf16=False):
    """``bf16``: a gemm mode (:func:`gemm_mode`); a lone layer knows the exact products and the bf16 operand mode only
    (modes 1 and 2 -> operand mode, mode 3 "fp32x3" -> exact)."""
    return GCNLayerFn.apply(x, adj, weight, bias, cut_len, relu, gemm_mode(bf16) in (1, 2), _wants_grad(x, weight, bias))


class PosEncMaskFn(torch.autograd.Function):
    """Positional_Encoder + Mask_Encoder + add (vision/model.py:229-232 etc.): (B,N,3),(B,N,1) -> (B,N,ld)."""

    @staticmethod
    def forward(ctx, verts, mask, packed, input_size, ld, gemm_bf16=False):
        L = _lib.load()
        verts, mask, packed = _req(verts, "verts"), _req(mask, "mask"), _req(packed, "pe_params")
        if packed.numel() != L.a3vt_posenc_param_count(input_size):
            raise RuntimeError("a3vt: packed positional-encoder parameter count mismatch")
        B, N, _ = verts.shape
        feats = torch.empty((B, N, ld), dtype=torch.float32, device=verts.device)
        ctx.wide_acts = None
        if input_size == 50:
            _lib.check(L.a3vt_posenc_mask_fwd(_lib.ptr(verts), _lib.ptr(mask), B * N, input_size, _lib.ptr(packed),
                                              _lib.ptr(feats), ld, _stream()), "posenc_mask_fwd")
        else:   # wide inputs (448 of the image models): three products on the matrix pipe, activations kept for the backward
            if not L.a3vt_posenc_wide_supported(input_size) or ld != input_size:
                raise RuntimeError(f"a3vt: vertex-feature encoder: input_size={input_size} ld={ld} unsupported")
            acts = torch.empty(L.a3vt_posenc_wide_acts_bytes(B * N, input_size), dtype=torch.uint8, device=verts.device)
            need_bwd = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]   # (grad mode is off inside forward)
            scratch = workspace("posenc", L.a3vt_posenc_wide_scratch_bytes(B * N, input_size, 0), verts.device)
            _lib.check(L.a3vt_posenc_wide_fwd(_lib.ptr(verts), _lib.ptr(mask), B * N, input_size, _lib.ptr(packed),
                                              _lib.ptr(feats), ld, _lib.ptr(acts), _lib.ptr(scratch), int(bool(gemm_bf16)),
                                              _stream()), "posenc_wide_fwd")
            ctx.wide_acts = acts if need_bwd else None
        ctx.save_for_backward(verts, mask, packed)
        ctx.dims = (input_size, ld)
        ctx.gemm_bf16 = int(bool(gemm_bf16))
        return feats

    @staticmethod
    def backward(ctx, gfeats):
        L = _lib.load()
        verts, mask, packed = ctx.saved_tensors
        input_size, ld = ctx.dims
        gfeats = _req(gfeats, "grad_feats")
        B, N, _ = verts.shape
        gverts = torch.empty_like(verts)
        gparams = torch.empty_like(packed)
        if input_size == 50:
            scratch = workspace("posenc", L.a3vt_posenc_scratch_bytes(B * N, input_size), verts.device)
            _lib.check(L.a3vt_posenc_mask_bwd(_lib.ptr(verts), _lib.ptr(mask), B * N, input_size, _lib.ptr(packed),
                                              _lib.ptr(gfeats), ld, _lib.ptr(gverts), _lib.ptr(gparams),
                                              _lib.ptr(scratch), _stream()), "posenc_mask_bwd")
        else:
            if ctx.wide_acts is None:
                raise RuntimeError("a3vt: vertex-feature encoder: backward without saved activations")
            scratch = workspace("posenc", L.a3vt_posenc_wide_scratch_bytes(B * N, input_size, 1), verts.device)
            _lib.check(L.a3vt_posenc_wide_bwd(_lib.ptr(verts), _lib.ptr(mask), B * N, input_size, _lib.ptr(packed),
                                              _lib.ptr(gfeats), ld, _lib.ptr(ctx.wide_acts), _lib.ptr(gverts),
                                              _lib.ptr(gparams), _lib.ptr(scratch), ctx.gemm_bf16, _stream()), "posenc_wide_bwd")
            ctx.wide_acts = None
        return gverts, None, gparams, None, None, None


class ImagePoolFn(torch.autograd.Function):
    """Image_Encoder.pooling (vision/model.py:70-103): verts (B,N,3) + feature maps (B,C_k,H_k,W_k) -> (B,N,sum C_k).
    Maps are consumed in torch's channels_last memory format (converted here if they are not already)."""

    @staticmethod
    def forward(ctx, verts, matrix, base, *maps):
        """``base`` (optional, (B,N,sum C_k) fp32): the result is ``base + pooled`` — the sum of vision/model.py:243,265,277 in
        the pooling's own pass (``a3vt_image_pool_fwd_add``); its gradient is the output gradient itself."""
        L = _lib.load()
        verts = _req(verts, "verts")
        B, N, _ = verts.shape
        cl = [m.contiguous(memory_format=torch.channels_last) for m in maps]
        for m in cl:
            if not m.is_cuda or m.dtype != torch.float32 or m.shape[0] != B:
                raise RuntimeError("a3vt: feature maps must be float32 (B,C,H,W) tensors on the GPU")
        chans = [int(m.shape[1]) for m in cl]
        ld = sum(chans)                                     # every C_k is a multiple of 4 (checked by the library)
        feats = torch.empty((B, N, ld), dtype=torch.float32, device=verts.device)
        if isinstance(matrix, torch.Tensor):               # host copy of the 3 x 4 camera matrix (a device tensor costs a sync)
            matrix = matrix.detach().cpu().reshape(-1).tolist()
        proj = (ctypes.c_float * 12)(*[float(x) for x in matrix])
        ints = lambda xs: (ctypes.c_int * len(xs))(*xs)  # noqa: E731
        geo = (ints(chans), ints([int(m.shape[2]) for m in cl]), ints([int(m.shape[3]) for m in cl]))
        if base is not None:
            base = _req(base, "base")
            if tuple(base.shape) != (B, N, ld):
                raise RuntimeError(f"a3vt: image_pool base must be {(B, N, ld)}, got {tuple(base.shape)}")
            _lib.check(L.a3vt_image_pool_fwd_add(_lib.ptr(verts), B, N, proj, len(cl), _ptr_array(cl), *geo, _lib.ptr(base),
                                                 _lib.ptr(feats), ld, _stream()), "image_pool_fwd_add")
        else:
            _lib.check(L.a3vt_image_pool_fwd(_lib.ptr(verts), B, N, proj, len(cl), _ptr_array(cl), *geo, _lib.ptr(feats), ld,
                                             _stream()), "image_pool_fwd")
        ctx.save_for_backward(verts, *cl)
        ctx.proj, ctx.geo, ctx.has_base = proj, geo, base is not None
        return feats

    @staticmethod
    def backward(ctx, gfeats):
        L = _lib.load()
        verts, *cl = ctx.saved_tensors
        B, N, _ = verts.shape
        gfeats = _req(gfeats, "grad_feats")
        gmaps = [torch.empty_like(m) for m in cl]          # keeps the channels_last strides
        gverts = torch.empty_like(verts)
        _lib.check(L.a3vt_image_pool_bwd(_lib.ptr(verts), B, N, ctx.proj, len(cl), _ptr_array(cl), *ctx.geo,
                                         _lib.ptr(gfeats), gfeats.shape[-1], _ptr_array(gmaps), _lib.ptr(gverts),
                                         _stream()), "image_pool_bwd")
        return (gverts, None, gfeats if ctx.has_base else None, *gmaps)


def image_pool(verts, matrix, maps, base=None):
    """Image_Encoder.pooling; with ``base``: ``base + pooling`` in one pass (the vertex-feature sum of the image models)."""
    return ImagePoolFn.apply(verts, matrix, base, *maps)


def bias_grad_nhwc(grad):
    """Sum of a (B,C,H,W) channels-last gradient over B, H, W -> fp32 (C,) (``a3vt_bias_grad_nhwc``)."""
    L = _lib.load()
    if not grad.is_cuda or grad.dim() != 4 or grad.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("a3vt: bias_grad_nhwc takes a float32 / bfloat16 (B,C,H,W) tensor on the GPU")
    g = grad.contiguous(memory_format=torch.channels_last)
    B, C, H, W = g.shape
    rows = B * H * W
    need = L.a3vt_bias_grad_scratch_bytes(rows, C)
    if need == 0:
        raise RuntimeError(f"a3vt: bias_grad_nhwc does not support {C} channels")
    scratch = torch.empty(need, dtype=torch.uint8, device=g.device)
    out = torch.empty(C, dtype=torch.float32, device=g.device)
    _lib.check(L.a3vt_bias_grad_nhwc(_lib.ptr(g), int(g.dtype == torch.bfloat16), rows, C, _lib.ptr(out), _lib.ptr(scratch),
                                     need, _stream()), "bias_grad_nhwc")
    return out


_BF16_COPIES = {}   # id(tensor) -> (weakref, version, data_ptr, optimizer epoch, bf16 copy)
_OPT_EPOCH = [0]    # moved by every torch optimizer step of the process once the cache is in use, and by invalidate_bf16_copies()
_BF16_HOOK = [None]  # None: not tried yet; True: the global step hook is registered; False: this torch has none (no caching)


def _optimizer_stepped(*_args, **_kwargs):
    _OPT_EPOCH[0] += 1


def invalidate_bf16_copies():
    """Forget every cached bf16 weight copy.  The cache notices in-place torch ops (``_version``), re-allocations
    (``data_ptr``) and optimizer steps (the step hook); writes through ``.data`` (``p.data.copy_``, ``.data.uniform_``) or a
    hand-written update move none of these and MUST be followed by this call — ``distributed.broadcast_parameters``,
    ``GCN_layer.reset_parameters`` and ``Engine.load`` (vision/train.py) do it themselves; ``load_state_dict`` alone is also
    caught (its ``copy_`` moves ``_version``)."""
    _OPT_EPOCH[0] += 1
    _BF16_COPIES.clear()


def _bf16_cache_on():
    """The process-wide optimizer post-step hook is registered on the FIRST use of the bf16 convolution branch, not at import
    (a host process that imports this module for the fp32 path gets no hook).  The trainer's optimizer — the library's one-launch
    Adam (optim.py) as well as torch's fused Adam — updates the weights in place WITHOUT moving their ``_version``; without a global step hook (older torch) nothing tells a
    stale copy from a fresh one, and every call casts."""
    if _BF16_HOOK[0] is None:
        try:
            from torch.optim.optimizer import register_optimizer_step_post_hook
            register_optimizer_step_post_hook(_optimizer_stepped)
            _BF16_HOOK[0] = True
        except ImportError:
            _BF16_HOOK[0] = False
    return _BF16_HOOK[0]


def _bf16_forget(key, ref):
    hit = _BF16_COPIES.get(key)
    if hit is not None and hit[0] is ref:       # the id can already belong to a new tensor with its own entry
        del _BF16_COPIES[key]


def _bf16_copy(t, channels_last):
    """bf16 (channels-last) copy of a convolution weight / bias, kept until the tensor can have changed: an in-place torch
    op (load_state_dict, copy_) moves ``t._version``; an optimizer step — neither the library's Adam nor torch's fused Adam moves it — moves the
    process-wide optimizer epoch (a global step post-hook); ``.data`` writers call :func:`invalidate_bf16_copies`.  A training
    loop casts once per step as before; the forward-only loops (validation, the K-candidate scoring of
    policies/environment.py:174-180) stop re-casting the 32 weights of the image pyramid on every call (64 copy launches per
    forward).  An entry dies with its tensor (weak-reference callback), so rebuilt models do not pin their copies."""
    on = _bf16_cache_on()
    key = id(t)
    hit = _BF16_COPIES.get(key) if on else None
    if (hit is not None and hit[0]() is t and hit[1] == t._version and hit[2] == t.data_ptr()
            and hit[3] == _OPT_EPOCH[0]):
        return hit[4]
    c = t.detach().to(torch.bfloat16)
    if channels_last:
        c = c.contiguous(memory_format=torch.channels_last)
    if on:
        ref = weakref.ref(t, lambda r, key=key: _bf16_forget(key, r))
        _BF16_COPIES[key] = (ref, t._version, t.data_ptr(), _OPT_EPOCH[0], c)
    return c


def prefetch_bf16_copies(items):
    """Refresh the cached bf16 copies of many convolution weights / biases at once: ``items`` = [(tensor, channels_last)].
    Everything whose cache entry is stale (see :func:`_bf16_copy`) is converted by ONE ``a3vt_cast_weights_bf16`` launch
    instead of two or three torch copy launches per tensor (84 per training step of the image model); the following
    :func:`_bf16_copy` calls hit the cache.  Tensors the kernel does not take (not fp32 / not contiguous) are left to them."""
    if not _bf16_cache_on():
        return
    stale = []
    for t, cl in items:
        hit = _BF16_COPIES.get(id(t))
        if (hit is not None and hit[0]() is t and hit[1] == t._version and hit[2] == t.data_ptr() and hit[3] == _OPT_EPOCH[0]):
            continue
        if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() in (1, 4):
            stale.append((t, cl))
    L = _lib.load()
    for i0 in range(0, len(stale), 96):
        part = stale[i0:i0 + 96]
        n = len(part)
        dsts = []
        for t, cl in part:
            fmt = torch.channels_last if (cl and t.dim() == 4) else torch.contiguous_format
            dsts.append(torch.empty(t.shape, dtype=torch.bfloat16, device=t.device, memory_format=fmt))
        src = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in part])
        dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
        outer = (ctypes.c_longlong * n)(*[t.shape[0] for t, _ in part])
        # a channels-last (O, I, KH, KW) tensor is [O][KH KW][I] in memory; everything else keeps its order (inner = 1)
        inner = (ctypes.c_int * n)(*[(t.shape[1] if (cl and t.dim() == 4) else 1) for t, cl in part])
        hw = (ctypes.c_int * n)(*[((t.shape[2] * t.shape[3]) if (cl and t.dim() == 4) else (t.numel() // t.shape[0])) for t, cl in part])
        _lib.check(L.a3vt_cast_weights_bf16(n, src, dst, outer, inner, hw, _stream()), "cast_weights_bf16")
        for (t, _), d in zip(part, dsts):
            key = id(t)
            ref = weakref.ref(t, lambda r, key=key: _bf16_forget(key, r))
            _BF16_COPIES[key] = (ref, t._version, t.data_ptr(), _OPT_EPOCH[0], d)


_CONV5_IMAGES = {}   # (id(weight), flip) -> (weakref, version, data_ptr, optimizer epoch, image); as _BF16_COPIES


def _conv5_image(weight, flip):
    """The bf16 A-fragment image of a (cout,cin,5,5) weight for ``a3vt_conv5_nhwc`` (``flip``: the input-gradient form), cached
    until the weight can have changed (same rules as :func:`_bf16_copy`)."""
    L = _lib.load()
    on = _bf16_cache_on()
    key = (id(weight), flip)
    hit = _CONV5_IMAGES.get(key) if on else None
    if (hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == weight.data_ptr() and hit[3] == _OPT_EPOCH[0]):
        return hit[4]
    w = _req(weight.detach(), "conv weight")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    img = torch.empty(L.a3vt_conv5_image_bytes(cout, cin, flip), dtype=torch.uint8, device=w.device)
    _lib.check(L.a3vt_conv5_weight_image(_lib.ptr(w), cout, cin, flip, _lib.ptr(img), _stream()), "conv5_weight_image")
    if on:
        ref = weakref.ref(weight, lambda r, key=key: _CONV5_IMAGES.pop(key, None))
        _CONV5_IMAGES[key] = (ref, weight._version, weight.data_ptr(), _OPT_EPOCH[0], img)
    return img


def conv5_nhwc(x, image, bias, cout, stride, pad):
    """``a3vt_conv5_nhwc`` on a channels-last bf16 (B,cin,H,W) tensor -> (B,cout,Ho,Wo), channels-last bf16."""
    L = _lib.load()
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - 5) // stride + 1, (W + 2 * pad - 5) // stride + 1
    y = torch.empty((B, cout, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    _lib.check(L.a3vt_conv5_nhwc(_lib.ptr(x), B, H, W, C, cout, stride, pad, _lib.ptr(image), _lib.ptr(bias), _lib.ptr(y), _stream()),
               "conv5_nhwc")
    return y


def conv5_supported(weight, stride, padding):
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (5, 5) or list(padding) != [1, 1] or stride[0] != stride[1]:
        return False
    return bool(_lib.load().a3vt_conv5_supported(int(weight.shape[1]), int(weight.shape[0]), int(stride[0])))


_CONV5F_FOLDS = {}   # id(conv.weight) -> (weakref, signature of every tensor read, optimizer epoch, image, scale, shift); as _BF16_COPIES


def bn_fold(conv_bias, bn):
    """Eval-mode ``BatchNorm2d`` after a convolution as the per-channel map ``y = scale * conv_without_bias(x) + shift``:
    ``scale = gamma / sqrt(running_var + eps)``, ``shift = beta + scale * (conv_bias - running_mean)``.  Plain tensor
    arithmetic in the dtype of the module's tensors (any device)."""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    mean = bn.running_mean if conv_bias is None else bn.running_mean - conv_bias.detach()
    return scale, bn.bias.detach() - scale * mean


def _conv5f_operands(conv, bn):
    """(weight image, scale, shift) of ``a3vt_conv5f_nhwc`` for a convolution and the eval-mode BatchNorm that follows it
    (``bn`` None: scale NULL, shift = the bias), cached until one of the tensors can have changed — the rules of
    :func:`_bf16_copy`: ``_version`` and ``data_ptr`` of every tensor read, and the process-wide optimizer epoch."""
    L = _lib.load()
    on = _bf16_cache_on()
    w = conv.weight
    read = [w, conv.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])
    sig = tuple((id(t), t._version, t.data_ptr()) for t in read if t is not None) + ((bn.eps,) if bn is not None else ())
    key = id(w)
    hit = _CONV5F_FOLDS.get(key) if on else None
    if hit is not None and hit[0]() is w and hit[1] == sig and hit[2] == _OPT_EPOCH[0]:
        return hit[3], hit[4], hit[5]
    wd = _req(w.detach(), "conv weight")
    cout, cin = int(wd.shape[0]), int(wd.shape[1])
    img = torch.empty(L.a3vt_conv5f_image_bytes(cin, cout), dtype=torch.uint8, device=wd.device)
    _lib.check(L.a3vt_conv5f_weight_image(_lib.ptr(wd), cout, cin, _lib.ptr(img), _stream()), "conv5f_weight_image")
    if bn is not None:
        scale, shift = bn_fold(conv.bias, bn)
        scale, shift = _req(scale, "folded scale"), _req(shift, "folded shift")
    else:
        scale, shift = None, (None if conv.bias is None else _req(conv.bias.detach(), "conv bias"))
    if on:
        ref = weakref.ref(w, lambda r, key=key: _CONV5F_FOLDS.pop(key, None))
        _CONV5F_FOLDS[key] = (ref, sig, _OPT_EPOCH[0], img, scale, shift)
    return img, scale, shift


def conv5f_supported(conv):
    w = conv.weight
    return (tuple(w.shape[2:]) == (5, 5) and conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1]
            and isinstance(conv.padding[0], int) and 0 <= conv.padding[0] <= 4 and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and bool(_lib.load().a3vt_conv5f_supported(int(w.shape[1]), int(w.shape[0]), int(conv.stride[0]))))


def conv5f(x_nhwc, conv, bn=None, relu=False):
    """``relu(bn(conv(x)))`` of an fp32 5 x 5 ``nn.Conv2d`` (+ an eval-mode ``nn.BatchNorm2d`` or None) on a channels-last
    ``(B,H,W,cin)`` tensor -> ``(B,Ho,Wo,cout)``: ``a3vt_conv5f_nhwc`` (csrc/conv5f.hip), exact fp32 on the matrix pipe with the
    BatchNorm folded into the epilogue.  Forward only: the result carries no autograd graph.  A shape the kernel does not take
    is an error, not a detour."""
    L = _lib.load()
    if bn is not None and (bn.training or not bn.track_running_stats):
        raise RuntimeError("a3vt: conv5f folds an eval-mode BatchNorm (running statistics); this one is in training mode")
    if not conv5f_supported(conv):
        raise RuntimeError(f"a3vt: conv5f does not take {conv}")
    x = _req(x_nhwc.detach(), "x")
    B, H, W, C = x.shape
    cout, stride, pad = int(conv.weight.shape[0]), int(conv.stride[0]), int(conv.padding[0])
    if C != conv.weight.shape[1]:
        raise RuntimeError(f"a3vt: conv5f: the map has {C} channels, the convolution takes {conv.weight.shape[1]}")
    img, scale, shift = _conv5f_operands(conv, bn)
    y = torch.empty((B, (H + 2 * pad - 5) // stride + 1, (W + 2 * pad - 5) // stride + 1, cout), dtype=torch.float32, device=x.device)
    _lib.check(L.a3vt_conv5f_nhwc(_lib.ptr(x), B, H, W, C, cout, stride, pad, _lib.ptr(img), _lib.ptr(scale), _lib.ptr(shift),
                                  int(bool(relu)), _lib.ptr(y), _stream()), "conv5f_nhwc")
    STATS["conv5f"] = STATS.get("conv5f", 0) + 1
    return y


LIBRARY_CONV5 = [True]   # layers 2-6 of the bf16 image branch on a3vt_conv5_nhwc (False: MIOpen, for A/B)
LIBRARY_CONV5_WRW = [True]   # their weight gradients on a3vt_conv5_weight_grad (False: MIOpen's split-K kernel + fill + cast)
_CONV5_WRW_SCRATCH = {}   # (device index, stream) -> scratch of a3vt_conv5_weight_grad (per-workgroup partial images)


def _conv5_weight_grad(xb, gy, weight, stride, padding, wb):
    """fp32 (cout,cin,5,5) weight gradient of a layer ``conv5_supported`` takes, from the layer's channels-last bf16
    input ``xb`` and output gradient ``gy``: ``a3vt_conv5_weight_grad`` (fixed summation order, no fill / cast launches)."""
    if not LIBRARY_CONV5_WRW[0]:
        return torch.ops.aten.convolution_backward(gy, xb, wb, None, stride, padding, [1, 1], False, [0, 0], 1, [False, True, False])[1]
    L = _lib.load()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    key = (xb.device.index, int(torch.cuda.current_stream().cuda_stream))
    need = L.a3vt_conv5_wrw_scratch_bytes(32, 32)
    buf = _CONV5_WRW_SCRATCH.get(key)
    if buf is None:
        buf = torch.empty(need, dtype=torch.uint8, device=xb.device)
        _CONV5_WRW_SCRATCH[key] = buf
    gw = torch.empty((cout, cin, 5, 5), dtype=torch.float32, device=xb.device)
    B, _, H, W = xb.shape
    _lib.check(L.a3vt_conv5_weight_grad(_lib.ptr(xb), _lib.ptr(gy), B, H, W, cin, cout, int(stride[0]), _lib.ptr(gw), _lib.ptr(buf), need,
                                        _stream()), "conv5_weight_grad")
    STATS["conv5_weight_grad"] = STATS.get("conv5_weight_grad", 0) + 1
    return gw


class ConvNHWCFn(torch.autograd.Function):
    """``nn.Conv2d`` of the image pyramid (vision/model.py:15-23) in the channels-last bf16 branch: MIOpen's NHWC bf16
    kernels for the convolution and its data / weight gradients, the bias gradient from the library (torch's own column
    reduction of the channels-last output gradient takes 1.3 ms on the 3-channel full-resolution map)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, add_bias=True):
        """``add_bias=False``: the output feeds a training-mode BatchNorm only (``BNReLUFn(..., pre_bias=bias)``), which removes
        the shift again: the bias-add launch is skipped; the bias gradient is formed as before."""
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wb = _bf16_copy(weight, True)
        # layers 2-6 of the pyramid (16 -> 16 and 32 -> 32 at stride 1, 16 -> 32 at stride 2): the library's direct convolution
        ctx.own = (LIBRARY_CONV5[0] and conv5_supported(weight, stride, padding) and weight.dtype == torch.float32
                   and bias.dtype == torch.float32 and xb.shape[2] >= 3 and xb.shape[3] >= 3)
        if ctx.own:
            y = conv5_nhwc(xb, _conv5_image(weight, 0), _req(bias.detach(), "conv bias") if add_bias else None,
                           int(weight.shape[0]), int(stride[0]), 1)
            STATS["conv5_fwd"] = STATS.get("conv5_fwd", 0) + 1
            ctx.weight = weight
        else:
            y = torch.ops.aten.convolution(xb, wb, _bf16_copy(bias, False) if add_bias else None, stride, padding, [1, 1], False, [0, 0], 1)
        ctx.save_for_backward(xb, wb)
        ctx.conf = (stride, padding, x.dtype, weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, wb = ctx.saved_tensors
        stride, padding, xdt, wdt, bdt = ctx.conf
        gy = gy.contiguous(memory_format=torch.channels_last)
        own = ctx.own and gy.dtype == torch.bfloat16
        need_gx = ctx.needs_input_grad[0]
        if not own:
            gx, gw, _ = torch.ops.aten.convolution_backward(gy, xb, wb, None, stride, padding, [1, 1], False, [0, 0], 1, [need_gx, True, False])
        else:
            if need_gx and list(stride) == [1, 1] and ctx.weight.shape[1] != 3:
                # the input gradient is the same convolution on gy with the weights transposed and flipped, padding 3
                gx = conv5_nhwc(gy, _conv5_image(ctx.weight, 1), None, int(ctx.weight.shape[1]), 1, 3)
                STATS["conv5_input_grad"] = STATS.get("conv5_input_grad", 0) + 1
            elif (need_gx and list(stride) == [2, 2] and tuple(ctx.weight.shape[:2]) == (16, 3)
                  and xb.shape[2] == 2 * gy.shape[2] + 2 and xb.shape[3] == 2 * gy.shape[3] + 2):
                # layer 1 (3 -> 16, stride 2): its input gradient as a stride-1 convolution of gy read as if upsampled with zeros
                L = _lib.load()
                gx = torch.empty_like(xb, memory_format=torch.channels_last)
                _lib.check(L.a3vt_conv5_input_grad_3x16s2(_lib.ptr(gy), gy.shape[0], gy.shape[2], gy.shape[3],
                                                          _lib.ptr(_conv5_image(ctx.weight, 1)), _lib.ptr(gx), _stream()), "conv5_input_grad_3x16s2")
                STATS["conv5_input_grad_3x16s2"] = STATS.get("conv5_input_grad_3x16s2", 0) + 1
            elif need_gx:      # (16 -> 32 at stride 2, 3 -> 3: MIOpen)
                gx = torch.ops.aten.convolution_backward(gy, xb, wb, None, stride, padding, [1, 1], False, [0, 0], 1, [True, False, False])[0]
            else:
                gx = None
            gw = _conv5_weight_grad(xb, gy, ctx.weight, stride, padding, wb)
        cs = getattr(gy, "_a3vt_colsum", None)
        if cs is not None and cs[1] == gy._version and cs[2] == gy.data_ptr() and cs[0].numel() == gy.shape[1]:
            gb = cs[0]            # formed by BNReLUFn.backward while it wrote gy
            STATS["bias_grad_from_bnrelu"] = STATS.get("bias_grad_from_bnrelu", 0) + 1
        else:
            gb = bias_grad_nhwc(gy)
        return (gx.to(xdt) if gx is not None else None), gw.to(wdt, memory_format=torch.contiguous_format), gb.to(bdt), None, None, None


_BNRELU_SCRATCH = {}   # (device index, stream) -> zero-initialised scratch of a3vt_bnrelu_*; the launches leave it zero
_BNRELU_MAX_C = 1024


def _bnrelu_scratch(dev):
    L = _lib.load()
    key = (dev.index, int(torch.cuda.current_stream().cuda_stream))
    buf = _BNRELU_SCRATCH.get(key)
    if buf is None:
        buf = torch.zeros(L.a3vt_bnrelu_scratch_bytes(_BNRELU_MAX_C), dtype=torch.uint8, device=dev)
        _BNRELU_SCRATCH[key] = buf
    return buf


class BNReLUFn(torch.autograd.Function):
    """Training-mode ``nn.BatchNorm2d`` followed by ``nn.ReLU`` of a ``CNN_layer`` (vision/model.py:15-23) on a channels-last
    bf16 map: ``a3vt_bnrelu_fwd / _bwd``, two launches each way.  Updates the module's running statistics and
    ``num_batches_tracked`` in place like the module does.  Returns a channels-last bf16 tensor.  ``pre_bias``: the bias of the
    convolution in front when that convolution did NOT add it (``ConvNHWCFn(..., add_bias=False)``): batch statistics remove a
    per-channel shift, so the output is the same and only ``running_mean`` takes the bias."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, num_batches, eps, momentum, pre_bias=None):
        L = _lib.load()
        if not x.is_cuda or x.dim() != 4 or x.dtype != torch.bfloat16:
            raise RuntimeError("a3vt: bnrelu takes a bfloat16 (B,C,H,W) tensor on the GPU")
        x = x.contiguous(memory_format=torch.channels_last)
        B, C, H, W = x.shape
        if C > _BNRELU_MAX_C:
            raise RuntimeError(f"a3vt: bnrelu supports up to {_BNRELU_MAX_C} channels")
        rows = B * H * W
        gamma, beta = _req(gamma, "bn weight"), _req(beta, "bn bias")
        y = torch.empty_like(x, memory_format=torch.channels_last)
        save = torch.empty((4, C), dtype=torch.float32, device=x.device)
        scratch = _bnrelu_scratch(x.device)
        if pre_bias is not None:
            pre_bias = _req(pre_bias.detach(), "pre_bias")
        _lib.check(L.a3vt_bnrelu_fwd(_lib.ptr(x), rows, C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(pre_bias), float(eps), float(momentum),
                                     _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(num_batches),
                                     _lib.ptr(y), _lib.ptr(save), _lib.ptr(scratch), scratch.numel(), _stream()), "bnrelu_fwd")
        ctx.save_for_backward(x, save)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.load()
        x, save = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = gy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        gx = torch.empty_like(x, memory_format=torch.channels_last)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        colsum = torch.empty(C, dtype=torch.float32, device=x.device)
        scratch = _bnrelu_scratch(x.device)
        _lib.check(L.a3vt_bnrelu_bwd(_lib.ptr(gy), _lib.ptr(x), B * H * W, C, _lib.ptr(save), _lib.ptr(gx), _lib.ptr(dg),
                                     _lib.ptr(db), _lib.ptr(colsum), _lib.ptr(scratch), scratch.numel(), _stream()), "bnrelu_bwd")
        # x is a Conv2d output in the pyramid: that layer's bias gradient is the column sum of gx, which the dx launch formed
        # on its way (ConvNHWCFn.backward picks it up if THIS tensor, unmodified, arrives as its output gradient)
        gx._a3vt_colsum = (colsum, gx._version, gx.data_ptr())
        return gx, dg, db, None, None, None, None, None, None


class VertexUpdateFn(torch.autograd.Function):
    """vertices[:, :n_vision] += update[:, :n_vision] (vision/model.py:250,270,283), out of place."""

    @staticmethod
    def forward(ctx, verts, update, n_vision):
        L = _lib.load()
        verts, update = _req(verts, "verts"), _req(update, "update")
        B, N, _ = verts.shape
        out = torch.empty_like(verts)
        _lib.check(L.a3vt_vertex_update(_lib.ptr(verts), _lib.ptr(update), B, N, n_vision, _lib.ptr(out), _stream()),
                   "vertex_update")
        ctx.n_vision = n_vision
        return out

    @staticmethod
    def backward(ctx, g):
        nv = ctx.n_vision
        if nv == g.shape[1]:
            return g, g, None
        gu = g.clone()
        gu[:, nv:] = 0
        return g, gu, None


class SamplePointsFn(torch.autograd.Function):
    """batch_sample (utility/utils.py:152-187) for `draws` clouds at once: verts (B,N,3) -> (draws,B,num,3)."""

    @staticmethod
    def forward(ctx, verts, faces, num, draws, seed, offset, face_idx, u, v):
        L = _lib.load()
        verts = _req(verts, "verts")
        faces = _req(faces, "faces", torch.int32)
        B, N, _ = verts.shape
        F = faces.shape[0]
        dev = verts.device
        points = torch.empty((draws, B, num, 3), dtype=torch.float32, device=dev)
        cdf = None
        if face_idx is None:
            cdf = torch.empty((B, F), dtype=torch.float32, device=dev)
            _lib.check(L.a3vt_face_cdf(_lib.ptr(verts), _lib.ptr(faces), B, N, F, _lib.ptr(cdf), _stream()), "face_cdf")
            fi = torch.empty((draws, B, num), dtype=torch.int32, device=dev)
            uu = torch.empty((draws, B, num), dtype=torch.float32, device=dev)
            vv = torch.empty((draws, B, num), dtype=torch.float32, device=dev)
            _lib.check(L.a3vt_sample_points_fwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(cdf), B, N, F, draws, num,
                                                None, None, None, seed, offset, _lib.ptr(points), _lib.ptr(fi),
                                                _lib.ptr(uu), _lib.ptr(vv), _stream()), "sample_points_fwd")
        else:
            fi = _req(face_idx, "face_idx", torch.int32).reshape(draws, B, num)
            uu = _req(u, "u").reshape(draws, B, num)
            vv = _req(v, "v").reshape(draws, B, num)
            _lib.check(L.a3vt_sample_points_fwd(_lib.ptr(verts), _lib.ptr(faces), None, B, N, F, draws, num,
                                                _lib.ptr(fi), _lib.ptr(uu), _lib.ptr(vv), 0, 0, _lib.ptr(points),
                                                None, None, None, _stream()), "sample_points_fwd")
        ctx.save_for_backward(faces, fi, uu, vv)
        ctx.dims = (B, N, F, draws, num)
        return points

    @staticmethod
    def backward(ctx, gpoints):
        L = _lib.load()
        faces, fi, uu, vv = ctx.saved_tensors
        B, N, F, draws, num = ctx.dims
        gpoints = _req(gpoints, "grad_points")
        gverts = torch.empty((B, N, 3), dtype=torch.float32, device=gpoints.device)
        _lib.check(L.a3vt_sample_points_bwd(_lib.ptr(faces), B, N, F, draws, num, _lib.ptr(fi), _lib.ptr(uu),
                                            _lib.ptr(vv), _lib.ptr(gpoints), _lib.ptr(gverts), _stream()),
                   "sample_points_bwd")
        return gverts, None, None, None, None, None, None, None, None


def sample_points(verts, faces, num, draws, seed=0, offset=0, return_samples=False):
    """Forward-only area-weighted sampling on the Philox path; with ``return_samples`` also the draws themselves
    (face_idx int32, u, v — each (draws,B,num)), e.g. to re-inject them into another call."""
    L = _lib.load()
    verts = _req(verts, "verts")
    faces = _req(faces, "faces", torch.int32)
    B, N, _ = verts.shape
    F = faces.shape[0]
    dev = verts.device
    points = torch.empty((draws, B, num, 3), dtype=torch.float32, device=dev)
    cdf = torch.empty((B, F), dtype=torch.float32, device=dev)
    fi = torch.empty((draws, B, num), dtype=torch.int32, device=dev)
    uu = torch.empty((draws, B, num), dtype=torch.float32, device=dev)
    vv = torch.empty((draws, B, num), dtype=torch.float32, device=dev)
    _lib.check(L.a3vt_face_cdf(_lib.ptr(verts), _lib.ptr(faces), B, N, F, _lib.ptr(cdf), _stream()), "face_cdf")
    _lib.check(L.a3vt_sample_points_fwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(cdf), B, N, F, draws, num, None, None,
                                        None, seed, offset, _lib.ptr(points), _lib.ptr(fi), _lib.ptr(uu), _lib.ptr(vv),
                                        _stream()), "sample_points_fwd")
    return (points, fi, uu, vv) if return_samples else points


# Search algorithm ChamferFn asks the library for (include/a3vt.h: a3vt_chamfer_fwd_ws): 0 = let it choose.  All of them
# return the same bits; tests flip this to prove it end to end.
CHAMFER_ALGO = 0


class ChamferFn(torch.autograd.Function):
    """pytorch3d chamfer_distance(x, y, batch_reduction=None) averaged over draws (utility/utils.py:204-217).
    x (draws,B,P,3), y (B,Q,3) -> cd (B,).  Forward-only callers may pass y (E,Q,3) with B a multiple of E: mesh b is compared
    with y[b % E] (the candidate-major batches of ``policies/scoring.py``: the ground truth is sorted once, not per candidate)."""

    @staticmethod
    def forward(ctx, x, y):
        L = _lib.load()
        x, y = _req(x, "x"), _req(y, "y")
        draws, B, P, _ = x.shape
        Q = y.shape[1]
        E = y.shape[0]
        if E != B and (E <= 0 or B % E != 0):
            raise RuntimeError("a3vt: chamfer batch mismatch (a shared ground truth needs B % E == 0)")
        dev = x.device
        dxy = torch.empty((draws, B, P), dtype=torch.float32, device=dev)
        ixy = torch.empty((draws, B, P), dtype=torch.int32, device=dev)
        dyx = torch.empty((draws, B, Q), dtype=torch.float32, device=dev)
        iyx = torch.empty((draws, B, Q), dtype=torch.int32, device=dev)
        cd = torch.empty((B,), dtype=torch.float32, device=dev)
        nbytes = L.a3vt_chamfer_workspace_bytes(draws, B, P, Q)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _lib.check(L.a3vt_chamfer_fwd_shared(_lib.ptr(x), _lib.ptr(y), draws, B, E, P, Q, _lib.ptr(dxy), _lib.ptr(ixy),
                                             _lib.ptr(dyx), _lib.ptr(iyx), _lib.ptr(cd), _lib.ptr(ws), nbytes, CHAMFER_ALGO,
                                             _stream()), "chamfer_fwd")
        ctx.save_for_backward(x, y, ixy, iyx)
        ctx.aux = (dxy, dyx)
        return cd

    @staticmethod
    def backward(ctx, gcd):
        L = _lib.load()
        x, y, ixy, iyx = ctx.saved_tensors
        draws, B, P, _ = x.shape
        Q = y.shape[1]
        if y.shape[0] != B:
            raise RuntimeError("a3vt: the shared-ground-truth Chamfer (y with fewer clouds than x has meshes) is forward-only "
                               "(scoring under no_grad); repeat y for a differentiable call")
        gcd = _req(gcd, "grad_cd")
        gx = torch.empty_like(x)
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        _lib.check(L.a3vt_chamfer_bwd(_lib.ptr(x), _lib.ptr(y), draws, B, P, Q, _lib.ptr(ixy), _lib.ptr(iyx),
                                      _lib.ptr(gcd), _lib.ptr(gx), _lib.ptr(gy), _stream()), "chamfer_bwd")
        return gx, gy


NN_ALGOS = {"auto": 0, "two_pass": 1, "sweep": 2, "pruned": 3}


def chamfer_nn(x, y, single_pass=True, algo=None):
    """Raw nearest-neighbour outputs (dist_xy, idx_xy, dist_yx, idx_yx, cd) — used by tests and scoring.
    ``algo``: "auto" | "two_pass" | "sweep" | "pruned" (include/a3vt.h: a3vt_chamfer_fwd_ws); by default the brute-force
    sweep, or with ``single_pass=False`` the two-pass search (no scratch).  The results are identical bit for bit."""
    L = _lib.load()
    x, y = _req(x, "x"), _req(y, "y")
    draws, B, P, _ = x.shape
    Q = y.shape[1]
    E = y.shape[0]                     # E < B: shared ground truth, mesh b against y[b % E] (a3vt_chamfer_fwd_shared)
    dev = x.device
    dxy = torch.empty((draws, B, P), dtype=torch.float32, device=dev)
    ixy = torch.empty((draws, B, P), dtype=torch.int32, device=dev)
    dyx = torch.empty((draws, B, Q), dtype=torch.float32, device=dev)
    iyx = torch.empty((draws, B, Q), dtype=torch.int32, device=dev)
    cd = torch.empty((B,), dtype=torch.float32, device=dev)
    if algo is None:
        algo = "sweep" if single_pass else "two_pass"
    nbytes = L.a3vt_chamfer_workspace_bytes(draws, B, P, Q) if algo != "two_pass" else 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    _lib.check(L.a3vt_chamfer_fwd_shared(_lib.ptr(x), _lib.ptr(y), draws, B, E, P, Q, _lib.ptr(dxy), _lib.ptr(ixy),
                                         _lib.ptr(dyx), _lib.ptr(iyx), _lib.ptr(cd), _lib.ptr(ws), nbytes, NN_ALGOS[algo],
                                         _stream()), "chamfer_fwd")
    return dxy, ixy, dyx, iyx, cd


class FoldFn(torch.autograd.Function):
    """One FoldingNet fold, conv3(relu(conv2(relu(bias_s + W1g g)))), on ``a3vt_fold_fwd/bwd`` (csrc/fold.hip): no
    (B * P) x 512 tensor exists in memory, forward or backward.  ``bias_s`` (B, 512) is conv1's code part, computed by torch
    outside (autograd carries its gradient on to the code and to that slice of the weight); ``g`` (B, P, k), k = 2 or 3;
    ``w1g`` (512, k), ``w2`` (512, 512), ``b2`` (512,), ``w3`` (3, 512), ``b3`` (3,) -> y (B, P, 3)."""

    @staticmethod
    def forward(ctx, bias_s, g, w1g, w2, b2, w3, b3):
        if isinstance(g, torch.Tensor) and g.dim() == 3 and g.shape[2] == 2 and g.requires_grad:
            # dg exists for k = 3 only; a None from backward would read as a zero gradient
            raise RuntimeError("a3vt: fold: the k = 2 lattice has no gradient path")
        L = _lib.load()
        bias_s, g, w1g, w2, b2, w3, b3 = (_req(t, n) for t, n in ((bias_s, "bias_s"), (g, "g"), (w1g, "w1g"), (w2, "w2"), (b2, "b2"),
                                                                  (w3, "w3"), (b3, "b3")))
        B, P, k = g.shape
        width = w2.shape[0]
        if bias_s.shape != (B, width) or w1g.shape != (width, k) or w2.shape != (width, width) or b2.shape != (width,) or \
                w3.shape != (3, width) or b3.shape != (3,):
            raise RuntimeError("a3vt: fold operand shapes disagree")
        y = torch.empty((B, P, 3), dtype=torch.float32, device=g.device)
        need = L.a3vt_fold_workspace_bytes(B, P, 0)
        ws = workspace("fold", need, g.device)
        _lib.check(L.a3vt_fold_fwd(_lib.ptr(bias_s), _lib.ptr(g), k, _lib.ptr(w1g), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(w3), _lib.ptr(b3),
                                   B, P, width, _lib.ptr(y), _lib.ptr(ws), need, _stream()), "fold_fwd")
        ctx.save_for_backward(bias_s, g, w1g, w2, b2, w3)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.load()
        bias_s, g, w1g, w2, b2, w3 = ctx.saved_tensors
        B, P, k = g.shape
        width = w2.shape[0]
        dy = _req(dy, "grad_y")
        dev = g.device
        dbias = torch.empty_like(bias_s)
        dg = torch.empty_like(g) if k == 3 and ctx.needs_input_grad[1] else None
        dw1g, dw2, db2, dw3 = torch.empty_like(w1g), torch.empty_like(w2), torch.empty_like(b2), torch.empty_like(w3)
        db3 = torch.empty((3,), dtype=torch.float32, device=dev)
        need = L.a3vt_fold_workspace_bytes(B, P, 1)
        ws = workspace("fold", need, dev)
        _lib.check(L.a3vt_fold_bwd(_lib.ptr(bias_s), _lib.ptr(g), k, _lib.ptr(w1g), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(w3), _lib.ptr(dy),
                                   B, P, width, _lib.ptr(dbias), _lib.ptr(dg), _lib.ptr(dw1g), _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(dw3),
                                   _lib.ptr(db3), _lib.ptr(ws), need, _stream()), "fold_bwd")
        return dbias, dg, dw1g, dw2, db2, dw3, db3


def fold(code, g, conv1, conv2, conv3):
    """A fold of ``FoldingNetDec`` on the fused kernels: ``code`` (B, 512), ``g`` (B, P, k), the fold's three ``Conv1d`` modules
    (their parameters stay whole: conv1.weight is sliced here) -> (B, P, 3)."""
    width = conv2.weight.shape[0]
    w1 = conv1.weight.squeeze(-1)
    bias_s = torch.addmm(conv1.bias, code, w1[:, :width].t())
    return FoldFn.apply(bias_s, g, w1[:, width:], conv2.weight.squeeze(-1), conv2.bias, conv3.weight.squeeze(-1), conv3.bias)


class DDQNTDFn(torch.autograd.Function):
    """The double-DQN target, loss and loss gradient on ``a3vt_ddqn_td`` / ``a3vt_ddqn_td_bwd`` (csrc/ddqn.hip): one launch each,
    no host sync.  Only ``q_cur`` carries a gradient."""

    @staticmethod
    def forward(ctx, q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, budget, gamma):
        L = _lib.load()
        q_cur, q_no, q_nt, mask = (_req(t, n) for t, n in ((q_cur, "q_cur"), (q_next_online, "q_next_online"),
                                                           (q_next_target, "q_next_target"), (mask, "mask")))
        actions, rewards = _req(actions, "actions"), _req(rewards, "rewards")
        denom = None if denom is None else _req(denom, "denom")
        B, A = q_cur.shape
        if q_no.shape != (B, A) or q_nt.shape != (B, A) or mask.shape != (B, A) or actions.shape != (B,) or rewards.shape != (B,) or \
                (denom is not None and denom.shape != (B,)):
            raise RuntimeError("a3vt: ddqn_td operand shapes disagree")
        dev = q_cur.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        diff, target = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
        best = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(L.a3vt_ddqn_td(_lib.ptr(q_cur), _lib.ptr(q_no), _lib.ptr(q_nt), _lib.ptr(mask), _lib.ptr(actions), _lib.ptr(rewards),
                                  _lib.ptr(denom), B, A, int(budget), float(gamma), _lib.ptr(loss), _lib.ptr(diff), _lib.ptr(best),
                                  _lib.ptr(target), _stream()), "ddqn_td")
        ctx.save_for_backward(diff, actions)
        ctx.shape = (B, A)
        ctx.mark_non_differentiable(best, target)
        return loss, best, target

    @staticmethod
    def backward(ctx, gloss, _gbest, _gtarget):
        L = _lib.load()
        diff, actions = ctx.saved_tensors
        B, A = ctx.shape
        gloss = _req(gloss, "grad_loss")
        dq = torch.empty((B, A), dtype=torch.float32, device=diff.device)
        _lib.check(L.a3vt_ddqn_td_bwd(_lib.ptr(diff), _lib.ptr(actions), _lib.ptr(gloss), B, A, _lib.ptr(dq), _stream()), "ddqn_td_bwd")
        return dq, None, None, None, None, None, None, None, None


def _ddqn_td_torch(q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, budget, gamma):
    """The same rule on torch ops (CPU tensors: the latent model, the host tests)."""
    not_done = mask.sum(dim=1) < budget - 1
    if denom is not None:
        rewards = rewards / denom
    act = actions.long().clamp(0, q_cur.shape[1] - 1)      # as the kernel: an action outside the table stays inside the row
    q = q_cur.gather(1, act.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        best = q_next_online.detach().masked_fill(mask > 0, -1e10).max(1)[1]
        nxt = q_next_target.detach().gather(1, best.unsqueeze(1)).squeeze(1)
        target = gamma * torch.where(not_done, nxt, torch.zeros_like(nxt)) + rewards
    return ((q - target) ** 2).mean(), best.to(torch.int32), target


def ddqn_td(q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, budget, gamma):
    """The reference's double-DQN update rule (policies/DDQN/ddqn.py:88-115) -> (loss, best_next int32 [B], target [B]).
    ``q_next_online`` is the UNPENALISED online next-state output: the ``-1e10`` where ``mask > 0`` is applied here.
    ``denom``: ``first_score`` / ``score`` for the reference's reward normalisations, or None.  GPU tensors run one launch
    (B <= 4096, A <= 304); CPU tensors take the same rule on torch ops."""
    if not q_cur.is_cuda:
        return _ddqn_td_torch(q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, budget, gamma)
    return DDQNTDFn.apply(q_cur, q_next_online.detach(), q_next_target.detach(), mask, actions, rewards, denom, budget, gamma)


# csrc/kernels.h's kLatentTile / kLatentQueryFloats / kLatentCachedRows (a3vt_latent_nn_tile() and its neighbours return the
# library's own; the tests choose their shapes around them): bank rows per workgroup of the distance kernel, floats of queries
# kept in LDS at a time, the largest bank the selection holds in registers.
LATENT_NN_TILE = 32
LATENT_NN_QUERY_FLOATS = 8192
LATENT_NN_CACHED_ROWS = 16384
LATENT_NN_MAX = dict(dim=4096, n_queries=1024, k=64, bank_rows=1 << 24, num_actions=304)


def _latent_nearest_check(bank, bank_actions, queries, taken, k):
    """Shapes, dtypes and limits of ``latent_nearest`` (both forms) -> (M, D, E, A)."""
    for t, name, dtype in ((bank, "bank", torch.float32), (queries, "queries", torch.float32), (taken, "taken", torch.float32),
                           (bank_actions, "bank_actions", torch.int32)):
        if t is None and name in ("taken", "bank_actions"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise RuntimeError(f"a3vt: latent_nearest `{name}` must be a {dtype} tensor")
        if t.device != bank.device:
            raise RuntimeError(f"a3vt: latent_nearest `{name}` is on {t.device}, the bank on {bank.device}")
    if bank.dim() != 2 or queries.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise RuntimeError(f"a3vt: latent_nearest wants bank (M, D) and queries (E, D), got {tuple(bank.shape)} and {tuple(queries.shape)}")
    (M, D), E = bank.shape, queries.shape[0]
    if bank_actions is not None and bank_actions.shape != (M,):
        raise RuntimeError(f"a3vt: latent_nearest bank_actions must be ({M},), got {tuple(bank_actions.shape)}")
    if taken is not None and (taken.dim() != 2 or taken.shape[0] != E):
        raise RuntimeError(f"a3vt: latent_nearest taken must be ({E}, num_actions), got {tuple(taken.shape)}")
    if taken is not None and bank_actions is None:
        raise RuntimeError("a3vt: latent_nearest taken without bank_actions")
    A = taken.shape[1] if taken is not None else LATENT_NN_MAX["num_actions"]     # (no mask: every action of the range qualifies)
    lim = LATENT_NN_MAX
    if not (1 <= D <= lim["dim"] and 1 <= E <= lim["n_queries"] and 1 <= int(k) <= lim["k"] and 1 <= M <= lim["bank_rows"]
            and 1 <= A <= lim["num_actions"]):
        raise RuntimeError(f"a3vt: latent_nearest bank_rows={M} dim={D} n_queries={E} num_actions={A} k={k} outside {lim}")
    return M, D, E, A


def _latent_nearest_torch(bank, bank_actions, queries, taken, k):
    """The contract of ``a3vt_latent_nearest`` on torch ops (CPU tensors: the host tests, the policy without a GPU): a stable
    sort by distance, so a tie goes to the lower row and NaN distances come last."""
    M, D, E, A = _latent_nearest_check(bank, bank_actions, queries, taken, k)
    k, k_eff = int(k), min(int(k), M)
    d = ((bank.unsqueeze(0) - queries.unsqueeze(1)) ** 2).mean(dim=2)                     # (E, M)
    sd, order = torch.sort(d, dim=1, stable=True)
    idx = torch.full((E, k), -1, dtype=torch.int32, device=bank.device)
    dist = torch.full((E, k), float("inf"), dtype=torch.float32, device=bank.device)
    idx[:, :k_eff], dist[:, :k_eff] = order[:, :k_eff].to(torch.int32), sd[:, :k_eff]
    if bank_actions is None:
        return idx, dist, None, None
    acts = bank_actions.long()[order[:, :k_eff]]                                          # (E, k_eff)
    ok = (acts >= 0) & (acts < A)
    if taken is not None:
        ok &= taken.gather(1, acts.clamp(0, A - 1)) == 0
    first = ok.int().argmax(dim=1)
    found = ok.any(dim=1)
    minus = torch.full((E,), -1, dtype=torch.int32, device=bank.device)
    action = torch.where(found, acts.gather(1, first.unsqueeze(1)).squeeze(1).to(torch.int32), minus)
    return idx, dist, action, torch.where(found, first.to(torch.int32), minus)


def latent_nearest(bank, bank_actions, queries, taken, k):
    """The nearest-neighbour policy's bank lookup (reference ``policies/NearestNeighbor/train.py:114-137``) ->
    ``(idx (E, k) int32, dist (E, k), action (E,) int32, rank (E,) int32)``: per query the ``min(k, M)`` nearest rows of ``bank``
    (M, D) by mean squared difference, nearest first, ties to the lower row, NaN last, padded with -1 / +inf; ``action`` is
    ``bank_actions`` (M,) int32 of the first listed row whose action is inside ``taken``'s (E, A) columns and not taken
    (``taken[e, a] == 0``), ``rank`` its position, both -1 when none qualifies.  ``taken`` None excludes nothing;
    ``bank_actions`` None gives a pure k-nearest query (``action`` and ``rank`` are None).  GPU tensors run
    ``a3vt_latent_nearest`` (csrc/latent_nn.hip: two launches, no host sync); CPU tensors take the same contract on torch ops."""
    if not bank.is_cuda:
        return _latent_nearest_torch(bank, bank_actions, queries, taken, k)
    M, D, E, A = _latent_nearest_check(bank, bank_actions, queries, taken, k)
    L = _lib.load()
    bank, queries = bank.contiguous(), queries.contiguous()
    bank_actions = None if bank_actions is None else bank_actions.contiguous()
    taken = None if taken is None else taken.contiguous()
    k, dev = int(k), bank.device
    idx = torch.empty((E, k), dtype=torch.int32, device=dev)
    dist = torch.empty((E, k), dtype=torch.float32, device=dev)
    action = rank = None
    if bank_actions is not None:
        action, rank = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
    scratch = workspace("latent_nn", L.a3vt_latent_nearest_scratch_bytes(E, M, k), dev)
    _lib.check(L.a3vt_latent_nearest(_lib.ptr(bank), _lib.ptr(bank_actions), M, D, _lib.ptr(queries), _lib.ptr(taken), E, A, k,
                                     _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(action), _lib.ptr(rank), _lib.ptr(scratch), _stream()),
               "latent_nearest")
    return idx, dist, action, rank


# csrc/kernels.h's kTallyMaxCandidates / kTallyMaxElements / kTallyMaxActions
CANDIDATE_TALLY_MAX = dict(K=304, E=1024, A=304)


def _candidate_tally_check(scores, candidates, first_score, taken, sums, checks, votes):
    """Shapes, dtypes and limits of ``candidate_tally`` (both forms) -> (K, E, A)."""
    def want(t, name, dtype):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"a3vt: candidate_tally `{name}` must be a {dtype} tensor, got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.device != scores.device and not (name == "candidates" and not t.is_cuda):
            raise ValueError(f"a3vt: candidate_tally `{name}` is on {t.device}, the scores on {scores.device}")
    want(scores, "scores", torch.float32)
    want(candidates, "candidates", torch.int32)
    if scores.dim() != 2 or candidates.shape != scores.shape:
        raise ValueError(f"a3vt: candidate_tally wants scores (K, E) and candidates (K, E), got {tuple(scores.shape)} and "
                         f"{tuple(candidates.shape)}")
    K, E = scores.shape
    state = [(t, name) for t, name in ((sums, "sums"), (checks, "checks"), (votes, "votes")) if t is not None]
    if (sums is None) != (checks is None):
        raise ValueError("a3vt: candidate_tally wants `sums` and `checks` together or neither")
    for t, name in state:
        want(t, name, torch.float64)
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"a3vt: candidate_tally `{name}` must be a contiguous (A,) tensor (it is updated in place), got "
                             f"{tuple(t.shape)}")
    if taken is not None:
        want(taken, "taken", torch.float32)
        if taken.dim() != 2 or taken.shape[0] != E:
            raise ValueError(f"a3vt: candidate_tally `taken` must be ({E}, A), got {tuple(taken.shape)}")
    widths = {name: int(t.shape[0]) for t, name in state}
    if taken is not None:
        widths["taken"] = int(taken.shape[1])
    if not widths:
        raise ValueError("a3vt: candidate_tally needs `taken` or a state tensor to know the number of actions A")
    A = next(iter(widths.values()))
    if any(w != A for w in widths.values()):
        raise ValueError(f"a3vt: candidate_tally: the number of actions differs: {widths}")
    if sums is not None:
        want(first_score, "first_score", torch.float32)
        if first_score.shape != (E,):
            raise ValueError(f"a3vt: candidate_tally `first_score` must be ({E},), got {tuple(first_score.shape)}")
    lim = CANDIDATE_TALLY_MAX
    if not (1 <= K <= lim["K"] and 1 <= E <= lim["E"] and 1 <= A <= lim["A"]):
        raise ValueError(f"a3vt: candidate_tally K={K} E={E} A={A} outside 1..{lim}")
    return K, E, A


def _candidate_tally_host(scores, candidates, first_score, taken, sums, checks, votes, unvisited):
    """The contract of ``a3vt_candidate_tally`` (include/a3vt.h) on NumPy views of CPU tensors: the choice as a stable
    lexicographic sort per element, the tally as the ordered walk it is."""
    K, E = scores.shape
    s, c = scores.numpy(), candidates.numpy()
    A = (sums if sums is not None else votes).shape[0] if taken is None else taken.shape[1]
    inside = (c >= 0) & (c < A)
    open_ = inside.copy()
    if taken is not None:
        open_ &= taken.numpy()[np.arange(E)[None, :], np.clip(c, 0, A - 1)] == 0
    nan = np.isnan(s)
    rank = np.where(open_, nan.astype(np.int64), 2)                       # eligible number < eligible NaN < not eligible
    value = np.where(nan | ~open_, 0.0, s.astype(np.float64))
    best = np.full(E, -1, dtype=np.int32)
    best_score = np.full(E, np.inf, dtype=np.float32)
    for e in range(E):
        k = np.lexsort((value[:, e], rank[:, e]))[0]                      # (stable: a tie, -0 == +0 included, goes to the lower k)
        if open_[k, e]:
            best[e], best_score[e] = c[k, e], s[k, e]
    if sums is not None:
        ratio = s / first_score.numpy()[None, :]                          # fp32 / fp32, correctly rounded
        acc, n = sums.numpy(), checks.numpy()
        for k in range(K):
            for e in range(E):
                a = c[k, e]
                if not inside[k, e]:
                    continue
                acc[a] = np.float64(ratio[k, e]) if acc[a] == unvisited else np.float64(np.float32(acc[a]) + ratio[k, e])
                n[a] += 1.0
    if votes is not None:
        v = votes.numpy()
        for e in range(E):
            if best[e] >= 0:
                v[best[e]] += 1.0
    return torch.from_numpy(best), torch.from_numpy(best_score)


def candidate_tally(scores, candidates, first_score, taken, sums=None, checks=None, votes=None, unvisited=1e10):
    """What the dataset-specific policies do with one swept batch's score table (reference ``policies/dataset_specific/LEBA.py:115-128``,
    ``MFBA.py:95-99``) -> ``(best (E,) int32, best_score (E,) float32)``.  ``scores`` (K, E) float32 and ``candidates`` (K, E)
    int32 (``candidates[k, e]``: the action candidate k tries on element e); ``taken`` (E, A) float32, non-zero = performed, or
    None.  ``best[e]`` is the candidate of the lowest score among the pairs ``taken`` leaves open (ties to the lower k, NaN after
    +inf, -1 / +inf when none is open).  ``sums`` / ``checks`` (A,) float64, updated IN PLACE: for k, then e, ascending, the
    fp32 ratio ``scores[k, e] / first_score[e]`` replaces a sum that equals ``unvisited`` and is otherwise added to it in fp32,
    and the action's count goes up by one.  ``votes`` (A,) float64, in place: one per element for its ``best``.  The whole
    contract is in ``include/a3vt.h``.  GPU tensors run ``a3vt_candidate_tally`` (csrc/candidate_tally.hip: one launch, no host
    synchronisation); CPU tensors take the same contract on NumPy.

    A table with a candidate outside ``[0, A)`` is refused.  ``candidates`` may stay on the host beside GPU ``scores`` (the
    policies build it there): it is then checked for free and uploaded.  A table already on the GPU is read back once for the
    check, which waits for the device."""
    K, E, A = _candidate_tally_check(scores, candidates, first_score, taken, sums, checks, votes)
    low, high = int(candidates.min()), int(candidates.max())
    if low < 0 or high >= A:
        raise ValueError(f"a3vt: candidate_tally: candidates outside [0, {A}): min {low}, max {high}")
    if not scores.is_cuda:
        return _candidate_tally_host(scores, candidates, first_score, taken, sums, checks, votes, float(unvisited))
    return _candidate_tally_launch(scores, candidates.to(scores.device), first_score, taken, sums, checks, votes, unvisited, K, E, A)


def _candidate_tally_launch(scores, candidates, first_score, taken, sums, checks, votes, unvisited, K, E, A):
    """The library call of ``candidate_tally`` on checked GPU tensors (the candidates' range is the caller's to vouch for)."""
    L = _lib.load()
    scores, candidates = scores.contiguous(), candidates.contiguous()
    first_score = None if first_score is None or sums is None else first_score.contiguous()
    taken = None if taken is None else taken.contiguous()
    best = torch.empty(E, dtype=torch.int32, device=scores.device)
    best_score = torch.empty(E, dtype=torch.float32, device=scores.device)
    _lib.check(L.a3vt_candidate_tally(_lib.ptr(scores), _lib.ptr(candidates), _lib.ptr(first_score), _lib.ptr(taken), K, E, A,
                                      float(unvisited), _lib.ptr(sums), _lib.ptr(checks), _lib.ptr(votes), _lib.ptr(best),
                                      _lib.ptr(best_score), _stream()), "candidate_tally")
    return best, best_score


def touch_assemble_launches(reset=False):
    """``a3vt_touch_assemble`` calls that launched since the last reset (a test hook, as ``voxel_launches``)."""
    return _launch_counts("a3vt_touch_assemble_launches", ("calls",), reset)


def touch_assemble(table_charts, table_codes, state_charts, state_masks, candidates, slot):
    """The touch charts and masks of K candidate action lists from the per-episode touch table, candidate-major, in the layout the
    reconstructor takes -> ``(charts (K, E, F * G * C, 3), masks (K, E, F * G * C, 1))``.  ``table_charts`` (E, A, F, C, 3)
    float32 and ``table_codes`` (E, A, F) int32 (2 = "touch", 1 = "no_touch", 0 = no contact: ``scoring.touch_slots``' codes);
    ``state_charts`` (E, F, G, C, 3) and ``state_masks`` (E, F, G, C, 1) or (E, F, G, C): the episode's touch state, left as it
    is; ``candidates`` (K, E): the action candidate k tries on element e.  Every block of the outputs is the state's, except
    grasp slot ``slot``, which holds the table's chart of the candidate's action and its code as a float.  Values move as bits.
    The whole contract is in ``include/a3vt.h``.  GPU tensors run ``a3vt_touch_assemble`` (csrc/touch_assemble.hip: one launch,
    no host synchronisation); CPU tensors take the same contract from torch indexing.

    ``candidates`` as a host sequence, array or CPU tensor is checked against ``[0, A)`` (``ValueError``) and uploaded once.  A
    GPU int32 tensor is not read back: the kernel gives an action outside ``[0, A)`` a zero chart and mask 0."""
    for t, name, dtype in ((table_charts, "table_charts", torch.float32), (table_codes, "table_codes", torch.int32),
                           (state_charts, "state_charts", torch.float32), (state_masks, "state_masks", torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"a3vt: touch_assemble `{name}` must be a {dtype} tensor, got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.device != table_charts.device:
            raise ValueError(f"a3vt: touch_assemble `{name}` is on {t.device}, the table on {table_charts.device}")
    if table_charts.dim() != 5 or table_charts.shape[4] != 3 or min(table_charts.shape) < 1:
        raise ValueError(f"a3vt: touch_assemble wants table_charts (E, A, F, C, 3), got {tuple(table_charts.shape)}")
    E, A, F, C, _ = table_charts.shape
    if table_codes.shape != (E, A, F):
        raise ValueError(f"a3vt: touch_assemble wants table_codes ({E}, {A}, {F}), got {tuple(table_codes.shape)}")
    if state_charts.dim() != 5 or state_charts.shape[2] < 1 or state_charts.shape != (E, F, state_charts.shape[2], C, 3):
        raise ValueError(f"a3vt: touch_assemble wants state_charts ({E}, {F}, G, {C}, 3), got {tuple(state_charts.shape)}")
    G = state_charts.shape[2]
    if tuple(state_masks.shape) not in ((E, F, G, C), (E, F, G, C, 1)):
        raise ValueError(f"a3vt: touch_assemble wants state_masks ({E}, {F}, {G}, {C}, 1), got {tuple(state_masks.shape)}")
    slot = int(slot)
    if not 0 <= slot < G:
        raise ValueError(f"a3vt: touch_assemble: slot={slot} outside [0, {G})")
    dev = table_charts.device
    if isinstance(candidates, torch.Tensor) and candidates.is_cuda:
        if candidates.dtype != torch.int32 or candidates.device != dev:
            raise ValueError(f"a3vt: touch_assemble: device `candidates` must be int32 on {dev}, got {candidates.dtype} on "
                             f"{candidates.device}")
        cand = candidates.contiguous()
    else:
        host = np.asarray(candidates.numpy() if isinstance(candidates, torch.Tensor) else candidates)
        if host.ndim != 2 or host.size == 0 or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"a3vt: touch_assemble wants integer candidates (K, {E}), got {host.dtype} {host.shape}")
        low, high = int(host.min()), int(host.max())
        if low < 0 or high >= A:
            raise ValueError(f"a3vt: touch_assemble: candidates outside [0, {A}): min {low}, max {high}")
        cand = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)
    if cand.dim() != 2 or cand.shape[1] != E or cand.shape[0] < 1:
        raise ValueError(f"a3vt: touch_assemble wants candidates (K, {E}), got {tuple(cand.shape)}")
    K = cand.shape[0]
    if K * E * F * G * C * 3 >= 1 << 31:
        raise ValueError(f"a3vt: touch_assemble: K*E*F*G*C*3={K * E * F * G * C * 3} is not below 2**31 (K={K} E={E} F={F} G={G} C={C})")
    if dev.type != "cuda":
        rows = cand.long()
        columns = torch.arange(E).unsqueeze(0).expand(K, E)
        charts = state_charts.unsqueeze(0).repeat(K, 1, 1, 1, 1, 1)
        masks = state_masks.reshape(1, E, F, G, C).repeat(K, 1, 1, 1, 1)
        charts[:, :, :, slot] = table_charts[columns, rows]
        masks[:, :, :, slot] = table_codes[columns, rows].clamp(0, 2).to(torch.float32).unsqueeze(-1)
        return charts.view(K, E, F * G * C, 3), masks.view(K, E, F * G * C, 1)
    table_charts, table_codes = table_charts.contiguous(), table_codes.contiguous()
    state_charts, state_masks = state_charts.contiguous(), state_masks.contiguous()
    charts = torch.empty((K, E, F * G * C, 3), dtype=torch.float32, device=dev)
    masks = torch.empty((K, E, F * G * C, 1), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().a3vt_touch_assemble(_lib.ptr(table_charts), _lib.ptr(table_codes), _lib.ptr(state_charts),
                                               _lib.ptr(state_masks), _lib.ptr(cand), K, E, A, F, G, C, slot, _lib.ptr(charts),
                                               _lib.ptr(masks), _stream()), "touch_assemble")
    return charts, masks


def chart_head_launches(reset=False):
    """``a3vt_touch_chart_head`` calls that launched since the last reset (a test hook, as ``touch_assemble_launches``)."""
    return _launch_counts("a3vt_touch_chart_head_launches", ("calls",), reset)


CHART_HEAD_SHAPES = ((256, 512), (128, 256), (75, 128))     # fc.0.0, fc.1.0, fc.2.0 of the touch ``Encoder``


def _chart_head_torch(features, fc, template, rot, pos, code):
    """The torch formulation of ``touch_chart_head``: the lines of ``Encoder.forward`` (``fc``, the template add,
    ``transform_verts``) and of ``scoring.touch_slots`` (the two ``where`` and the ``expand``), on any device."""
    n = features.shape[0]
    verts = template.view(1, -1, 3).repeat(n, 1, 1)
    verts = verts + fc(features).view(-1, verts.shape[1], 3)
    pred = torch.bmm(rot, verts.permute(0, 2, 1)).permute(0, 2, 1) + pos.view(-1, 1, 3)
    code = code.to(torch.float32).view(n, 1, 1)
    code = torch.where(code == 2, code, torch.where(code == 1, code, torch.zeros_like(code)))     # (any other code is 0)
    charts = torch.where(code == 2, pred, torch.where(code == 1, pos.view(n, 1, 3).expand_as(pred), torch.zeros_like(pred)))
    masks = code.expand(n, verts.shape[1], 1)
    return charts.contiguous(), masks.contiguous()


def touch_chart_head(features, fc, template, rot, pos, code, want_slots=False):
    """The head of the touch chart predictor and the slot rule of ``scoring.touch_slots`` for n views -> ``rows`` (n, 25, 4)
    float32: x, y, z, mask — the layout of a data set's ``touch_charts.npy``; with ``want_slots`` ``(rows, charts (n, 25, 3),
    masks (n, 25, 1))``, the two tensors ``touch_slots`` returns.

    ``features`` (n, 512) float32: ``Encoder.predict_features``; ``fc``: the encoder's ``fc`` (three ``Linear``, 512 -> 256 ->
    128 -> 75, ReLU after the first two); ``template`` (25, 3); ``rot`` (n, 3, 3), ``pos`` (n, 3): the finger frames; ``code``
    (n,) integers: 2 = "touch" (the predicted chart in the finger's frame, mask 2), 1 = "no_touch" (the finger's position 25
    times, mask 1), anything else zeros and mask 0.  A select: a NaN in the features of a view whose code is not 2 does not reach
    its rows.  Forward only: nothing carries an autograd graph.

    GPU tensors run ``a3vt_touch_chart_head`` (csrc/chart_head.hip: ONE launch, exact fp32 in a fixed order of every sum, so a
    view's rows are the same bits alone and inside any batch; the contract is in ``include/a3vt.h``).  CPU tensors take the torch
    lines the kernel replaces (``Encoder.forward`` + ``touch_slots``), bit for bit what those give."""
    layers = [fc[i][0] for i in range(3)]
    dev = features.device
    for t, name, shape in ((features, "features", (-1, CHART_HEAD_SHAPES[0][1])), (template, "template", (25, 3)),
                           (rot, "rot", (-1, 3, 3)), (pos, "pos", (-1, 3))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != len(shape) or \
                any(s != -1 and s != d for s, d in zip(shape, t.shape)):
            raise ValueError(f"a3vt: touch_chart_head wants `{name}` float32 {shape} (-1: n), got "
                             f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.device != dev:
            raise ValueError(f"a3vt: touch_chart_head `{name}` is on {t.device}, the features on {dev}")
    n = features.shape[0]
    if n < 1 or rot.shape[0] != n or pos.shape[0] != n:
        raise ValueError(f"a3vt: touch_chart_head wants n >= 1 views in features, rot and pos, got {n}, {rot.shape[0]}, {pos.shape[0]}")
    if not isinstance(code, torch.Tensor) or code.is_floating_point() or tuple(code.shape) != (n,) or code.device != dev:
        raise ValueError(f"a3vt: touch_chart_head wants `code` ({n},) integers on {dev}, got "
                         f"{(code.dtype, tuple(code.shape), code.device) if isinstance(code, torch.Tensor) else type(code).__name__}")
    for layer, shape in zip(layers, CHART_HEAD_SHAPES):
        if tuple(layer.weight.shape) != shape or layer.bias is None or layer.weight.dtype != torch.float32 or layer.weight.device != dev:
            raise ValueError(f"a3vt: touch_chart_head wants a float32 Linear {shape[1]} -> {shape[0]} with bias on {dev}, got {layer} "
                             f"({layer.weight.dtype} on {layer.weight.device})")
    if n * CHART_HEAD_SHAPES[0][1] >= 1 << 31:
        raise ValueError(f"a3vt: touch_chart_head: n*512={n * 512} is not below 2**31 (n={n})")
    with torch.no_grad():
        if dev.type != "cuda":
            charts, masks = _chart_head_torch(features, fc, template, rot, pos, code)
            rows = torch.cat((charts, masks), dim=-1)
            return (rows, charts, masks) if want_slots else rows

        def operand(t):                     # contiguous, and on a 16-byte boundary (a view into a larger tensor need not be)
            t = t.detach().contiguous()
            return t.clone() if t.data_ptr() % 16 else t
        weights = [operand(p) for layer in layers for p in (layer.weight, layer.bias)]
        features, template, rot, pos = operand(features), operand(template), operand(rot), operand(pos)
        code = code.to(torch.int32).contiguous()
        rows = torch.empty((n, 25, 4), dtype=torch.float32, device=dev)
        charts = torch.empty((n, 25, 3), dtype=torch.float32, device=dev) if want_slots else None
        masks = torch.empty((n, 25, 1), dtype=torch.float32, device=dev) if want_slots else None
        _lib.check(_lib.load().a3vt_touch_chart_head(_lib.ptr(features), *(_lib.ptr(w) for w in weights), _lib.ptr(template),
                                                     _lib.ptr(rot), _lib.ptr(pos), _lib.ptr(code), n, _lib.ptr(rows), _lib.ptr(charts),
                                                     _lib.ptr(masks), _stream()), "touch_chart_head")
    return (rows, charts, masks) if want_slots else rows


TOUCH_RES = 121                                    # csrc/kernels.h's kTouchRes
TOUCH_DEFAULTS = dict(max_depth=0.025, yfov=40.0 / 180.0 * np.pi, znear=1e-4, zfar=10.0)   # the reference's sensor and camera


def _touch_views(cam_pos, cam_rot):
    cam_pos, cam_rot = _req(cam_pos, "cam_pos"), _req(cam_rot, "cam_rot")
    I = cam_pos.shape[0]
    if cam_pos.shape != (I, 3) or cam_rot.shape != (I, 3, 3) or I < 1:
        raise ValueError(f"a3vt: touch_render wants cam_pos (I, 3) and cam_rot (I, 3, 3), I >= 1, got {tuple(cam_pos.shape)} and "
                         f"{tuple(cam_rot.shape)}")
    return cam_pos, cam_rot, I


def _touch_outputs(I, device, want_touch, want_points):
    pix = TOUCH_RES * TOUCH_RES
    touch = torch.empty((I, TOUCH_RES, TOUCH_RES, 3), dtype=torch.float32, device=device) if want_touch else None
    points = torch.empty((I, pix, 3), dtype=torch.float32, device=device) if want_points else None
    count = torch.empty(I, dtype=torch.int32, device=device) if want_points else None
    return touch, points, count, torch.empty(I, dtype=torch.int32, device=device)


def _touch_result(depth, touch, points, count, status):
    out = {"depth": depth, "status": status}
    if touch is not None:
        out["touch"] = touch
    if points is not None:
        out["points"], out["count"] = points, count
    return out


def touch_render(verts, faces, face_offset, image_mesh, cam_pos, cam_rot, max_depth=TOUCH_DEFAULTS["max_depth"],
                 yfov=TOUCH_DEFAULTS["yfov"], znear=TOUCH_DEFAULTS["znear"], zfar=TOUCH_DEFAULTS["zfar"], want_touch=True,
                 want_points=True):
    """The rendered touch sampler's signals for I finger views over a table of M meshes (reference ``simulator/scene/instance.py``
    ``:121-258``; ``a3vt_touch_render``, csrc/touch_render.hip: two launches on the current stream, no host synchronisation).
    ``verts`` (V, 3) float32 and ``faces`` (F, 3) int32 with global indices, ``face_offset`` (M + 1,) int32, ``image_mesh`` (I,)
    int32, ``cam_pos`` (I, 3) / ``cam_rot`` (I, 3, 3) float32: the finger frames as ``*_ref_frame.npy`` stores them.  Returns a dict:
    ``depth`` (I, 121, 121), ``status`` (I,) int32 (1 = "touch"), with ``want_touch`` ``touch`` (I, 121, 121, 3) in 0..255, with
    ``want_points`` ``points`` (I, 14641, 3) and ``count`` (I,) int32: view i's contact points are ``points[i, :count[i]]``, in
    row-major pixel order; the rows after them are not written.  The whole contract is in ``include/a3vt.h``."""
    verts, faces = _req(verts, "verts"), _req(faces, "faces", torch.int32)
    face_offset, image_mesh = _req(face_offset, "face_offset", torch.int32), _req(image_mesh, "image_mesh", torch.int32)
    cam_pos, cam_rot, I = _touch_views(cam_pos, cam_rot)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"a3vt: touch_render wants verts (V, 3) and faces (F, 3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if face_offset.dim() != 1 or face_offset.numel() < 2 or image_mesh.shape != (I,):
        raise ValueError(f"a3vt: touch_render wants face_offset (M + 1,), M >= 1, and image_mesh ({I},), got "
                         f"{tuple(face_offset.shape)} and {tuple(image_mesh.shape)}")
    depth = torch.empty((I, TOUCH_RES, TOUCH_RES), dtype=torch.float32, device=verts.device)
    touch, points, count, status = _touch_outputs(I, verts.device, want_touch, want_points)
    _lib.check(_lib.load().a3vt_touch_render(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(face_offset),
                                             face_offset.numel() - 1, _lib.ptr(image_mesh), _lib.ptr(cam_pos), _lib.ptr(cam_rot), I,
                                             float(max_depth), float(yfov), float(znear), float(zfar), _lib.ptr(depth), _lib.ptr(touch),
                                             _lib.ptr(points), _lib.ptr(count), _lib.ptr(status), _stream()), "touch_render")
    return _touch_result(depth, touch, points, count, status)


def touch_finish(depth, cam_pos, cam_rot, max_depth=TOUCH_DEFAULTS["max_depth"], yfov=TOUCH_DEFAULTS["yfov"], want_touch=True,
                 want_points=True):
    """``touch_render``'s second launch alone (``a3vt_touch_finish``) on depth maps (I, 121, 121) the caller supplies — recorded
    ones, or a test's: the same dict, ``depth`` as given."""
    depth = _req(depth, "depth")
    cam_pos, cam_rot, I = _touch_views(cam_pos, cam_rot)
    if depth.shape != (I, TOUCH_RES, TOUCH_RES):
        raise ValueError(f"a3vt: touch_finish wants depth ({I}, {TOUCH_RES}, {TOUCH_RES}), got {tuple(depth.shape)}")
    touch, points, count, status = _touch_outputs(I, depth.device, want_touch, want_points)
    _lib.check(_lib.load().a3vt_touch_finish(_lib.ptr(depth), _lib.ptr(cam_pos), _lib.ptr(cam_rot), I, float(max_depth), float(yfov),
                                             _lib.ptr(touch), _lib.ptr(points), _lib.ptr(count), _lib.ptr(status), _stream()),
               "touch_finish")
    return _touch_result(depth, touch, points, count, status)


def touch_pack_launches(reset=False):
    """``a3vt_touch_pack`` calls that launched since the last reset (a test hook, as ``touch_assemble_launches``)."""
    return _launch_counts("a3vt_touch_pack_launches", ("calls",), reset)


def touch_pack(out, want_touch=True, want_points=True, capacity=None):
    """What ``touch_render`` / ``touch_finish`` returned (``out``: that dict) in the form a data set stores it, on the device
    (``a3vt_touch_pack``, csrc/touch_pack.hip: ONE launch on the current stream, no host synchronisation) -> a dict with, under
    ``want_touch``, ``touch_u8`` (I, 121, 121, 3) uint8 — ``out["touch"]`` clamped to [0, 255] and truncated, NaN 0: for the
    renderer's values ``.to(torch.uint8)`` — and, under ``want_points``, ``offsets`` (I + 1,) int32, the exclusive prefix sum of
    ``n_i = count[i] if status[i] == 1 else 0``, and ``cloud`` (capacity, 3) float32 whose rows ``[offsets[i], offsets[i + 1])``
    are ``points[i, :n_i]`` bit for bit.  The rows from ``offsets[I]`` on are not written.

    ``capacity`` None sizes ``cloud`` for the worst case, I * 14641 rows, and nothing is read back.  With a bound the launch
    writes no row when the total exceeds it; this function then reads ``offsets[I]`` (one synchronisation) and raises
    ``RuntimeError``.  The whole contract is in ``include/a3vt.h``."""
    want_touch, want_points = bool(want_touch), bool(want_points)
    if not want_touch and not want_points:
        raise ValueError("a3vt: touch_pack: neither want_touch nor want_points")
    status = _req(out["status"], "status", torch.int32)
    I, dev, pix = status.shape[0], status.device, TOUCH_RES * TOUCH_RES
    if status.shape != (I,) or I < 1:
        raise ValueError(f"a3vt: touch_pack wants status (I,), I >= 1, got {tuple(status.shape)}")
    touch = points = count = touch_u8 = offsets = cloud = None
    if want_touch:
        if "touch" not in out:
            raise ValueError("a3vt: touch_pack: want_touch, but the render was made without want_touch")
        touch = _req(out["touch"], "touch")
        if touch.shape != (I, TOUCH_RES, TOUCH_RES, 3) or touch.device != dev:
            raise ValueError(f"a3vt: touch_pack wants touch ({I}, {TOUCH_RES}, {TOUCH_RES}, 3) on {dev}, got {tuple(touch.shape)} on "
                             f"{touch.device}")
        if touch.data_ptr() % 16:                       # (a view into a larger tensor need not sit on a 16-byte boundary)
            touch = touch.clone()
        touch_u8 = torch.empty((I, TOUCH_RES, TOUCH_RES, 3), dtype=torch.uint8, device=dev)
    if want_points:
        if "points" not in out or "count" not in out:
            raise ValueError("a3vt: touch_pack: want_points, but the render was made without want_points")
        points, count = _req(out["points"], "points"), _req(out["count"], "count", torch.int32)
        if points.shape != (I, pix, 3) or count.shape != (I,) or points.device != dev or count.device != dev:
            raise ValueError(f"a3vt: touch_pack wants points ({I}, {pix}, 3) and count ({I},) on {dev}, got {tuple(points.shape)} on "
                             f"{points.device} and {tuple(count.shape)} on {count.device}")
        rows = I * pix if capacity is None else int(capacity)
        if rows < 0:
            raise ValueError(f"a3vt: touch_pack: capacity={capacity} is negative")
        offsets = torch.empty(I + 1, dtype=torch.int32, device=dev)
        cloud = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    return _touch_pack_into(touch, points, count, status if want_points else None, I, touch_u8, offsets, cloud, capacity is not None)


def _touch_pack_into(touch, points, count, status, I, touch_u8, offsets, cloud, bounded):
    """The library call of ``touch_pack`` into buffers the caller made (tests hand in a pre-filled ``cloud``)."""
    rows = 0 if cloud is None else cloud.shape[0]
    _lib.check(_lib.load().a3vt_touch_pack(_lib.ptr(touch), _lib.ptr(points), _lib.ptr(count), _lib.ptr(status), I, rows,
                                           _lib.ptr(touch_u8), _lib.ptr(offsets), _lib.ptr(cloud) if rows else None, _stream()),
               "touch_pack")
    result = {}
    if touch_u8 is not None:
        result["touch_u8"] = touch_u8
    if offsets is not None:
        result["offsets"], result["cloud"] = offsets, cloud
        if bounded:
            total = int(offsets[I].item())
            if total > rows:
                raise RuntimeError(f"a3vt: touch_pack: the views hold {total} contact points, more than capacity={rows}; no row of "
                                   "cloud was written")
    return result


# ---- the finger closing of the kinematic grasp (csrc/grasp_close.hip; the rule is stated in include/a3vt.h) ----
GRASP_FINGERS, GRASP_CHAIN, GRASP_JOINTS, GRASP_TABLE_COLS = 4, 7, 4, 26     # csrc/kernels.h's kGrasp*
GRASP_LINKS = GRASP_FINGERS * GRASP_CHAIN
GRASP_MIN_AXIS2 = 1e-24                                                     # a cross-product axis shorter than this (squared) is skipped
GRASP_SLACK = 1e-4                                                          # csrc/grasp_close.hip's kGraspSlack


def grasp_launches(reset=False):
    """``a3vt_grasp_close`` calls that launched since the last reset, and the kernels they launched (a test hook)."""
    return _launch_counts("a3vt_grasp_launches", ("calls", "launches"), reset)


def grasp_limits():
    """``capacity`` (candidate triangles a workgroup of ``a3vt_grasp_close`` holds in LDS), ``per_launch`` (grasps of one launch)
    and ``table_cols``, from the library."""
    L = _lib.load()
    return dict(capacity=L.a3vt_grasp_limit(0), per_launch=L.a3vt_grasp_limit(1), table_cols=L.a3vt_grasp_limit(2))


def _grasp_tables(hand_table, q0):
    table = np.ascontiguousarray(hand_table.cpu().numpy() if isinstance(hand_table, torch.Tensor) else hand_table, np.float64)
    rest = np.ascontiguousarray(q0.cpu().numpy() if isinstance(q0, torch.Tensor) else q0, np.float64)
    if table.shape != (GRASP_LINKS, GRASP_TABLE_COLS) or rest.shape != (GRASP_LINKS,):
        raise ValueError(f"a3vt: grasp_close wants hand_table ({GRASP_LINKS}, {GRASP_TABLE_COLS}) and q0 ({GRASP_LINKS},), got "
                         f"{table.shape} and {rest.shape}")
    return table, rest


def grasp_reach(hand_table):
    """The four chains' reach radii as ``a3vt_grasp_close``'s cull uses them (``a3vt_grasp_reach``; host arithmetic, no GPU)."""
    table, _ = _grasp_tables(hand_table, np.zeros(GRASP_LINKS))
    out = [_lib.load().a3vt_grasp_reach(table.ctypes.data_as(ctypes.c_void_p), c) for c in range(GRASP_FINGERS)]
    if min(out) < 0:
        _lib.check(-1, "grasp_reach")
    return out


def _grasp_rotation(axis, angle):
    x, y, z = axis
    c, s = np.cos(angle), np.sin(angle)
    t = 1.0 - c
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y], [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


def _grasp_chain_from(rows, base_pos, base_rot, angles, first, pos, rot):
    """The poses of the chain's links ``first``.. from their parents' (``pos`` / ``rot`` hold the links before ``first``), in place."""
    for k in range(first, GRASP_CHAIN):
        t = rows[k]
        parent = int(t[0])
        p, R = (base_pos, base_rot) if parent < 0 else (pos[parent], rot[parent])
        pos[k] = p + R @ t[2:5]
        rot[k] = R @ t[5:14].reshape(3, 3)
        if t[1]:
            rot[k] = rot[k] @ _grasp_rotation(t[14:17], angles[k])


def _grasp_overlap(centre, axes, half, tri):
    """Any overlap between the boxes (centre (b, 3), axes (b, 3, 3) with the box's axes as columns, half (b, 3)) and the triangles
    (n, 3, 3): the 13-axis test in each box's frame, all pairs at once."""
    if len(tri) == 0 or len(centre) == 0:
        return False
    p = np.einsum("bji,bnkj->bnki", axes, tri[None] - centre[:, None, None, :])          # (b, n, vertex, component)
    h = half[:, None, :]
    if not ((p.min(axis=2) <= h) & (p.max(axis=2) >= -h)).all(axis=-1).any():
        return False
    e = p[:, :, [1, 2, 0]] - p                                                              # p1 - p0, p2 - p1, p0 - p2
    candidates = [np.cross(e[:, :, 0], e[:, :, 1])]
    for j in range(3):
        ex, ey, ez = e[:, :, j, 0], e[:, :, j, 1], e[:, :, j, 2]
        zero = np.zeros_like(ex)
        candidates += [np.stack((zero, -ez, ey), -1), np.stack((ez, zero, -ex), -1), np.stack((-ey, ex, zero), -1)]
    a = np.stack(candidates, axis=2)                                                        # (b, n, 10, 3)
    d = np.einsum("bnai,bnki->bnak", a, p)
    r = np.einsum("bnai,bi->bna", np.abs(a), half)
    separated = ((a * a).sum(-1) >= GRASP_MIN_AXIS2) & ((d.min(-1) > r) | (d.max(-1) < -r))
    inside = ((p.min(axis=2) <= h) & (p.max(axis=2) >= -h)).all(axis=-1)
    return bool((inside & ~separated.any(-1)).any())


def _grasp_reach_host(rows):
    path, reach = np.zeros(GRASP_CHAIN), 0.0
    for k in range(GRASP_CHAIN):
        if k > 0:
            path[k] = path[int(rows[k][0])] + np.linalg.norm(rows[k][2:5])
        if rows[k][19]:
            reach = max(reach, path[k] + np.linalg.norm(rows[k][20:23]) + np.linalg.norm(rows[k][23:26]))
    return reach


def _grasp_close_host(verts, faces, face_offset, grasp_mesh, base_pos, base_rot, table, q0, steps):
    """The rule of ``a3vt_grasp_close`` in float64 NumPy, a query's boxes and triangles all at once."""
    G, V = len(grasp_mesh), len(verts)
    q_out, blocked = np.zeros((G, 16)), np.zeros((G, 16), np.int32)
    link_pos, link_rot = np.zeros((G, GRASP_LINKS, 3)), np.zeros((G, GRASP_LINKS, 3, 3))
    triangles = {}
    for g in range(G):
        m = int(grasp_mesh[g])
        if m not in triangles:
            f = faces[int(face_offset[m]):int(face_offset[m + 1])]
            f = f[((f >= 0) & (f < V)).all(axis=1)] if len(f) else f.reshape(0, 3)
            tri = verts[f].reshape(-1, 3, 3)
            tri = tri[np.isfinite(tri).all(axis=(1, 2))]
            mid = tri.mean(axis=1)
            triangles[m] = (tri, mid, np.linalg.norm(tri - mid[:, None, :], axis=2).max(axis=1) if len(tri) else np.zeros(0))
        tri, mid, spread = triangles[m]
        for c in range(GRASP_FINGERS):
            rows = table[c * GRASP_CHAIN:(c + 1) * GRASP_CHAIN].copy()
            rows[1:, 0] -= c * GRASP_CHAIN                                                  # parents within the chain
            angles = q0[c * GRASP_CHAIN:(c + 1) * GRASP_CHAIN].copy()
            upper, delta = rows[:, 18], (rows[:, 18] - angles) / steps
            pos, rot = np.zeros((GRASP_CHAIN, 3)), np.zeros((GRASP_CHAIN, 3, 3))
            _grasp_chain_from(rows, base_pos[g], base_rot[g], angles, 0, pos, rot)
            near = np.linalg.norm(mid - pos[0], axis=1) <= _grasp_reach_host(rows) + GRASP_SLACK + spread
            cand, cand_mid, cand_spread = tri[near], mid[near], spread[near]
            boxed = rows[:, 19] != 0
            size = np.linalg.norm(rows[:, 23:26], axis=1)
            took = np.full(GRASP_JOINTS, steps, np.int32)
            frozen = np.zeros(GRASP_JOINTS, bool)
            for step in range(1, steps + 1):
                if frozen.all():
                    break
                for j in range(GRASP_JOINTS):
                    if frozen[j]:
                        continue
                    tried = angles.copy()
                    tried[j] = upper[j] if step == steps else q0[c * GRASP_CHAIN + j] + step * delta[j]
                    hit = False
                    if len(cand):
                        tp, tr = pos.copy(), rot.copy()
                        _grasp_chain_from(rows, base_pos[g], base_rot[g], tried, j, tp, tr)
                        links = [k for k in range(j, GRASP_CHAIN) if boxed[k]]
                        centre = np.array([tp[k] + tr[k] @ rows[k][20:23] for k in links]).reshape(-1, 3)
                        close = np.zeros(len(cand), bool)
                        for b, k in enumerate(links):
                            close |= np.linalg.norm(cand_mid - centre[b], axis=1) <= size[k] + cand_spread + GRASP_SLACK
                        if close.any():
                            hit = _grasp_overlap(centre, tr[links], rows[links, 23:26], cand[close])
                    if hit:
                        frozen[j], took[j] = True, step - 1
                    else:
                        angles = tried
                        if len(cand):
                            pos, rot = tp, tr
            if not len(cand):
                _grasp_chain_from(rows, base_pos[g], base_rot[g], angles, 0, pos, rot)
            q_out[g, 4 * c:4 * c + 4], blocked[g, 4 * c:4 * c + 4] = angles[:GRASP_JOINTS], took
            link_pos[g, c * GRASP_CHAIN:(c + 1) * GRASP_CHAIN], link_rot[g, c * GRASP_CHAIN:(c + 1) * GRASP_CHAIN] = pos, rot
    last = [c * GRASP_CHAIN + GRASP_CHAIN - 1 for c in range(GRASP_FINGERS)]
    return q_out, blocked, link_pos, link_rot, link_pos[:, last], link_rot[:, last]


def grasp_candidates(verts, faces, face_offset, grasp_mesh, base_pos, base_rot, hand_table):
    """(G, 4) int64: per (grasp, finger) the triangles that pass the cull of ``a3vt_grasp_close`` — the count its workgroup holds in
    LDS up to ``grasp_limits()["capacity"]`` — formed on the host in float32 with the kernel's test (arrays or tensors; a
    measuring and test aid: a triangle within float32 rounding of the sphere may be counted differently)."""
    f32 = np.float32
    as_np = lambda a, dtype: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype)  # noqa: E731
    verts, faces, base_pos, base_rot = as_np(verts, f32), as_np(faces, np.int64), as_np(base_pos, f32), as_np(base_rot, f32)
    table, _ = _grasp_tables(hand_table, np.zeros(GRASP_LINKS))
    reach = grasp_reach(table)
    counts = np.zeros((len(grasp_mesh), GRASP_FINGERS), np.int64)
    for g, m in enumerate(np.asarray(grasp_mesh).tolist()):
        f = faces[int(face_offset[m]):int(face_offset[m + 1])]
        f = f[((f >= 0) & (f < len(verts))).all(axis=1)] if len(f) else f.reshape(0, 3)
        tri = verts[f].reshape(-1, 3, 3)
        mid = (tri[:, 0] + tri[:, 1] + tri[:, 2]) * f32(1.0 / 3.0)
        spread = np.sqrt(((tri - mid[:, None, :]) ** 2).sum(-1).max(axis=1)) if len(tri) else np.zeros(0, f32)
        for c in range(GRASP_FINGERS):
            centre = base_pos[g] + base_rot[g].reshape(3, 3) @ table[c * GRASP_CHAIN, 2:5].astype(f32)
            with np.errstate(invalid="ignore"):
                counts[g, c] = int((np.sqrt(((mid - centre) ** 2).sum(-1)) <= f32(reach[c]) + f32(GRASP_SLACK) + spread).sum())
    return counts


def grasp_close(verts, faces, face_offset, grasp_mesh, base_pos, base_rot, hand_table, q0, steps=64):
    """The finger closing of G placed hands over a table of M meshes (``a3vt_grasp_close``, csrc/grasp_close.hip: one launch per 64
    grasps on the current stream, no host synchronisation; the rule and the table's columns are stated in ``include/a3vt.h``).
    **A kinematic stand-in for the reference's five ``stepSimulation`` calls under position control, not pybullet: no frame of it
    has been compared with one of pybullet's.**

    ``verts`` (V, 3) float32 and ``faces`` (F, 3) int32 with global indices (``touch_render``'s layout); ``face_offset`` (M + 1,)
    and ``grasp_mesh`` (G,): lists, arrays or tensors, read on the host; ``base_pos`` (G, 3) / ``base_rot`` (G, 3, 3) float32;
    ``hand_table`` (28, 26) and ``q0`` (28,) float64 (``HandModel.table()`` / ``.q0``).  Returns a dict: ``q`` (G, 16) float32 and
    ``blocked_step`` (G, 16) int32 (entry 4 c + j: joint j of finger c), ``link_pos`` (G, 28, 3), ``link_rot`` (G, 28, 3, 3),
    ``frame_pos`` (G, 4, 3), ``frame_rot`` (G, 4, 3, 3) float32.

    GPU tensors run the kernel in float32.  CPU tensors take the same rule in float64 NumPy (the results are then float64 but
    for ``blocked_step``): the pattern of ``voxel_surface``, for hosts without a GPU and for tests."""
    table, rest = _grasp_tables(hand_table, q0)
    steps = int(steps)
    to_list = lambda a: [int(x) for x in (a.tolist() if hasattr(a, "tolist") else a)]  # noqa: E731
    face_offset, grasp_mesh = to_list(face_offset), to_list(grasp_mesh)
    G, M = len(grasp_mesh), len(face_offset) - 1
    if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or \
            faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("a3vt: grasp_close wants tensors verts (V, 3) and faces (F, 3)")
    if tuple(base_pos.shape) != (G, 3) or tuple(base_rot.shape) != (G, 3, 3):
        raise ValueError(f"a3vt: grasp_close wants base_pos ({G}, 3) and base_rot ({G}, 3, 3), got {tuple(base_pos.shape)} and "
                         f"{tuple(base_rot.shape)}")
    names = ("q", "blocked_step", "link_pos", "link_rot", "frame_pos", "frame_rot")
    if not verts.is_cuda:
        F = faces.shape[0]
        if steps < 1 or M < 1 or face_offset[0] < 0 or any(b < a for a, b in zip(face_offset, face_offset[1:])) or face_offset[-1] > F \
                or any(not 0 <= m < M for m in grasp_mesh):
            raise ValueError(f"a3vt: grasp_close: steps={steps} must be >= 1, face_offset={face_offset} must start at >= 0, not "
                             f"decrease and end at <= F={F}, and grasp_mesh must lie in 0..{M - 1}")
        out = _grasp_close_host(verts.detach().numpy().astype(np.float64), faces.numpy().astype(np.int64), face_offset, grasp_mesh,
                                np.asarray(base_pos, np.float64).reshape(G, 3), np.asarray(base_rot, np.float64).reshape(G, 3, 3), table,
                                rest, steps)
        return {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in zip(names, out)}
    dev = verts.device
    verts, faces = _req(verts, "verts"), _req(faces, "faces", torch.int32)
    base_pos, base_rot = _req(base_pos, "base_pos"), _req(base_rot, "base_rot")
    offsets, which = np.array(face_offset, np.int32), np.array(grasp_mesh if G else [0], np.int32)
    out = (torch.empty((G, 16), dtype=torch.float32, device=dev), torch.empty((G, 16), dtype=torch.int32, device=dev),
           torch.empty((G, GRASP_LINKS, 3), dtype=torch.float32, device=dev), torch.empty((G, GRASP_LINKS, 3, 3), dtype=torch.float32, device=dev),
           torch.empty((G, GRASP_FINGERS, 3), dtype=torch.float32, device=dev),
           torch.empty((G, GRASP_FINGERS, 3, 3), dtype=torch.float32, device=dev))
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_grasp_close(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], host(offsets), M,
                                                host(which), _lib.ptr(base_pos) if G else None, _lib.ptr(base_rot) if G else None, G,
                                                host(table), host(rest), steps, *((_lib.ptr(t) if G else None) for t in out), _stream()),
                   "grasp_close")
    return dict(zip(names, out))


# ---- the hand's placement on the convex hull without a hull (csrc/hull_place.hip; the rule is stated in include/a3vt.h) ----
HULL_MAX_ACTIONS, HULL_GJK_PASSES, HULL_PIVOT_PASSES = 128, 32, 64          # csrc/kernels.h's kHull*
HULL_FLAT, HULL_MIN_SIN2 = 1e-12, 1e-24


def hull_place_launches(reset=False):
    """``a3vt_hull_place`` calls that launched since the last reset, and the kernels they launched (a test hook)."""
    return _launch_counts("a3vt_hull_place_launches", ("calls", "launches"), reset)


def _cross2(p, q):
    return p[0] * q[1] - p[1] * q[0]


def _hull_place_steps(V, d, hand_distance, tip, largest):
    """The rule of ``a3vt_hull_place`` for one (mesh, action) as a generator: it yields the normal of the next support pass, is
    sent ``(w, hi, lo)`` — the lowest index of the largest ``n . v_i``, that value and the smallest — and returns
    ``(status, base_pos, base_rot, simplex, t)``.  Scalar float64 steps in the kernel's order, operation for operation."""
    none = (np.zeros(3), np.zeros((3, 3)), (-1, -1, -1), 0.0)
    dot = lambda n, v: (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]  # noqa: E731
    k = 0 if abs(d[0]) <= abs(d[1]) and abs(d[0]) <= abs(d[2]) else 1 if abs(d[1]) <= abs(d[2]) else 2
    e = np.zeros(3)
    e[k] = 1.0
    x = np.array([d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]])
    x = x / np.sqrt(dot(x, x))
    y = np.array([d[1] * x[2] - d[2] * x[1], d[2] * x[0] - d[0] * x[2], d[0] * x[1] - d[1] * x[0]])
    y = y / np.sqrt(dot(y, y))
    proj = lambda i: (dot(V[i], x), dot(V[i], y))  # noqa: E731
    lift = lambda u: np.array([u[0] * x[0] + u[1] * y[0], u[0] * x[1] + u[1] * y[1], u[0] * x[2] + u[1] * y[2]])  # noqa: E731
    # phase 1: a triangle whose projection holds the origin
    ia, _, _ = yield x
    pa = proj(ia)
    if pa[0] < 0.0:
        return (1,) + none
    if pa[0] == 0.0:
        return (2,) + none
    u = (-pa[0], -pa[1])
    ib, _, _ = yield lift(u)
    pb = proj(ib)
    sv = pb[0] * u[0] + pb[1] * u[1]
    if sv < 0.0:
        return (1,) + none
    if sv == 0.0 or ib == ia:
        return (2,) + none
    for step in range(HULL_GJK_PASSES):
        ex, ey = pb[0] - pa[0], pb[1] - pa[1]
        orient = ey * pa[0] - ex * pa[1]
        if orient == 0.0 and step > 0:           # (on the opening edge the origin lies between a and b: see the header)
            return (2,) + none
        u = (-ey, ex) if orient >= 0.0 else (ey, -ex)
        ic, _, _ = yield lift(u)
        pc = proj(ic)
        sv = pc[0] * u[0] + pc[1] * u[1]
        if sv < 0.0:
            return (1,) + none
        if sv == 0.0 or ic == ia or ic == ib:
            return (2,) + none
        ac, bc = (pc[0] - pa[0], pc[1] - pa[1]), (pc[0] - pb[0], pc[1] - pb[1])
        o_ac, b_ac = _cross2(ac, (-pa[0], -pa[1])), _cross2(ac, (pb[0] - pa[0], pb[1] - pa[1]))
        o_bc, a_bc = _cross2(bc, (-pb[0], -pb[1])), _cross2(bc, (pa[0] - pb[0], pa[1] - pb[1]))
        if o_ac == 0.0 or o_bc == 0.0 or b_ac == 0.0 or a_bc == 0.0:
            return (2,) + none
        if (o_ac > 0.0) != (b_ac > 0.0):         # the origin is outside edge a c: b leaves
            ib, pb = ic, pc
        elif (o_bc > 0.0) != (a_bc > 0.0):       # outside edge b c: a leaves
            ia, pa = ic, pc
        else:
            break
    else:
        return (2,) + none
    # phase 2: pivots to the optimal basis
    for _ in range(HULL_PIVOT_PASSES):
        a, b, c = V[ia], V[ib], V[ic]
        e1, e2 = (b[0] - a[0], b[1] - a[1], b[2] - a[2]), (c[0] - a[0], c[1] - a[1], c[2] - a[2])
        N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        den = dot(N, d)
        if den == 0.0:
            return (2,) + none
        n = np.array([N[0] / den, N[1] / den, N[2] / den])
        t = dot(n, a)
        w, hi, lo = yield n
        if hi <= t or w == ia or w == ib or w == ic:
            break
        pw = proj(w)
        area = _cross2((pb[0] - pa[0], pb[1] - pa[1]), (pc[0] - pa[0], pc[1] - pa[1]))
        if area == 0.0:
            return (2,) + none
        rel = lambda p, q: (p[0] - q[0], p[1] - q[1])  # noqa: E731
        lam = [max(_cross2(pb, pc) / area, 0.0), max(_cross2(pc, pa) / area, 0.0), max(_cross2(pa, pb) / area, 0.0)]
        mu = [_cross2(rel(pb, pw), rel(pc, pw)) / area, _cross2(rel(pc, pw), rel(pa, pw)) / area, _cross2(rel(pa, pw), rel(pb, pw)) / area]
        leave, best = -1, 0.0
        for j in range(3):
            if mu[j] > 0.0 and (leave < 0 or lam[j] / mu[j] < best):
                leave, best = j, lam[j] / mu[j]
        if leave < 0:
            return (2,) + none
        if leave == 0:
            ia, pa = w, pw
        elif leave == 1:
            ib, pb = w, pw
        else:
            ic, pc = w, pw
    else:
        return (2,) + none
    # the checks
    if t <= 0.0:
        return (1,) + none
    if hi - lo <= HULL_FLAT * largest:
        return (2,) + none
    # the pose: place_hand line for line
    point = np.array([d[0] * t, d[1] * t, d[2] * t])
    length = np.sqrt(dot(N, N))
    normal = np.array([N[0] / length, N[1] / length, N[2] / length])
    moved = point + normal * 0.0001
    if dot(point, point) > dot(moved, moved):
        normal = -normal
    position = point + normal * hand_distance
    normal = normal - 0.001
    length = np.sqrt(dot(normal, normal))
    bx, by, bz = normal[0] / length, normal[1] / length, normal[2] / length
    v = (0.0, bz, -by)                                  # (-1, 0, 0) x b
    cosine, sin2 = -bx, bz * bz + by * by
    if sin2 < HULL_MIN_SIN2:
        return (2,) + none
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    f = (1.0 - cosine) / sin2
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            kk = (K[i, 0] * K[0, j] + K[i, 1] * K[1, j]) + K[i, 2] * K[2, j]
            R[i, j] = ((1.0 if i == j else 0.0) + K[i, j]) + kk * f
    base = np.array([position[i] - ((R[i, 0] * tip[0] + R[i, 1] * tip[1]) + R[i, 2] * tip[2]) for i in range(3)])
    return 0, base, R, (int(ia), int(ib), int(ic)), float(t)


def _hull_place_host(verts, vert_offset, directions, hand_distance, tip):
    """The rule of ``a3vt_hull_place`` in float64 NumPy: per mesh every action's scalar steps run side by side, and each round's
    support passes are one (V, actions) product."""
    M, A = len(vert_offset) - 1, len(directions)
    status, t = np.ones((M, A), np.int32), np.zeros((M, A))
    base_pos, base_rot, simplex = np.zeros((M, A, 3)), np.zeros((M, A, 3, 3)), np.full((M, A, 3), -1, np.int32)
    for m in range(M):
        V = verts[vert_offset[m]:vert_offset[m + 1]].astype(np.float64)
        if len(V) < 4 or not np.isfinite(V).all():
            continue
        largest = float(np.abs(V).max())
        runs = {a: _hull_place_steps(V, directions[a], hand_distance, tip, largest) for a in range(A)}
        asks = {a: next(run) for a, run in runs.items()}
        while asks:
            who = sorted(asks)
            n = np.array([asks[a] for a in who])                                              # (k, 3)
            values = (V[:, 0:1] * n[:, 0] + V[:, 1:2] * n[:, 1]) + V[:, 2:3] * n[:, 2]        # (V, k), the kernel's order
            w, lo = values.argmax(axis=0), values.min(axis=0)
            asks = {}
            for j, a in enumerate(who):
                try:
                    asks[a] = runs[a].send((int(w[j]), float(values[w[j], j]), float(lo[j])))
                except StopIteration as done:
                    status[m, a], base_pos[m, a], base_rot[m, a], simplex[m, a], t[m, a] = done.value
    return status, base_pos, base_rot, simplex, t


def hull_place(verts, vert_offset, directions, hand_distance=0.013, tip_offset=(0.0, 0.0, 0.133)):
    """The hand's base pose for every one of A actions on every one of M meshes (``a3vt_hull_place``, csrc/hull_place.hip: one
    workgroup per (mesh, action), one launch per 128 meshes on the current stream, no host synchronisation).  It is the placement of
    ``simulator.physics.grasping.place_hand`` without a hull: the farthest point of the ray along ``directions[a]`` in the convex
    hull of the mesh's vertices is a linear programme in three variables, solved by support queries over the vertices in float64
    (``include/a3vt.h`` states the rule in full).

    ``verts`` (V, 3) float32; ``vert_offset`` (M + 1,) and ``directions`` (A, 3): lists, arrays or tensors, read on the host.
    Returns a dict: ``status`` (M, A) int32 — 0 placed, 1 no intersection (``place_hand``'s None), 2 not decided here (ask
    ``place_hand``) — ``base_pos`` (M, A, 3), ``base_rot`` (M, A, 3, 3) float32, ``simplex`` (M, A, 3) int32 (the facet's vertices,
    indices within the mesh) and ``t`` (M, A) float64 (the hit is ``t * direction``).  Rows with status != 0 are zeros, simplex -1.

    GPU tensors run the kernel.  CPU tensors take the same rule in float64 NumPy (``base_pos`` / ``base_rot`` are then float64):
    the pattern of ``grasp_close``, for hosts without a GPU and for tests."""
    as_np = lambda a, dtype: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype)  # noqa: E731
    offsets, dirs, tip = as_np(vert_offset, np.int64).reshape(-1), as_np(directions, np.float64), as_np(tip_offset, np.float64).reshape(-1)
    hand_distance = float(hand_distance)
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("a3vt: hull_place wants a tensor verts (V, 3)")
    if dirs.ndim != 2 or dirs.shape[1] != 3 or tip.shape != (3,) or len(offsets) < 2:
        raise ValueError(f"a3vt: hull_place wants vert_offset (M + 1,), directions (A, 3) and tip_offset (3,), got {offsets.shape}, "
                         f"{dirs.shape} and {tip.shape}")
    M, A, V = len(offsets) - 1, len(dirs), verts.shape[0]
    names = ("status", "base_pos", "base_rot", "simplex", "t")
    if not verts.is_cuda:
        if not 1 <= A <= HULL_MAX_ACTIONS or offsets[0] < 0 or (np.diff(offsets) < 0).any() or offsets[-1] > V or \
                not (np.isfinite(dirs).all() and np.isfinite(tip).all() and np.isfinite(hand_distance)) or not dirs.any(axis=1).all():
            raise ValueError(f"a3vt: hull_place: A={A} must lie in 1..{HULL_MAX_ACTIONS}, vert_offset must start at >= 0, not decrease "
                             f"and end at <= V={V}, and directions, tip_offset and hand_distance must be finite, no direction zero")
        out = _hull_place_host(verts.detach().numpy(), offsets, dirs, hand_distance, tip)
        return {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in zip(names, out)}
    dev = verts.device
    verts = _req(verts, "verts")
    offsets = offsets.astype(np.int32)
    out = (torch.empty((M, A), dtype=torch.int32, device=dev), torch.empty((M, A, 3), dtype=torch.float32, device=dev),
           torch.empty((M, A, 3, 3), dtype=torch.float32, device=dev), torch.empty((M, A, 3), dtype=torch.int32, device=dev),
           torch.empty((M, A), dtype=torch.float64, device=dev))
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_hull_place(_lib.ptr(verts) if V else None, V, host(offsets), M, host(dirs), A, hand_distance, host(tip),
                                               *(_lib.ptr(t) for t in out), _stream()), "hull_place")
    return dict(zip(names, out))


# The reference's vision scene (simulator/rendering/vision_renderer.py:35-77): the camera 0.4243 from the origin and looking at it,
# pyrender's default background as RENDER_DEFAULTS has it, the object's colour, four point lights (x, y, z, intensity).
VISION_DEFAULTS = dict(yfov=60.0 / 180.0 * np.pi, znear=0.01, zfar=10.0, width=256, height=256,
                       cam_pos=(-0.3, 0.0, 0.3), cam_euler_xyz_deg=(45.0, 0.0, 270.0),
                       lights=((0.0, -0.8, 0.3, 1.0), (0.0, 0.8, 0.3, 1.0), (-1.0, 0.0, 1.0, 1.0), (1.0, 0.0, 1.0, 1.0)),
                       ambient=0.3, colour=(228, 217, 111), background=(255, 255, 255))

# The reference's camera, lights and colours (utility/pretty_render.py:35-76, :129): what CameraRenderer starts from.
RENDER_DEFAULTS = dict(yfov=60.0 / 180.0 * np.pi, znear=0.01, zfar=10.0, width=512, height=512,
                       cam_pos=(0.0, 0.6, 0.6), cam_euler_xyz_deg=(45.0, 0.0, 180.0),
                       lights=((0.0, -0.8, 0.3, 1.8), (0.0, 0.8, 0.3, 1.8), (-1.0, 0.0, 1.0, 1.8), (1.0, 0.0, 1.0, 1.8)),
                       ambient=0.3, colour=(228, 217, 111), background=(255, 255, 255))
SCENE_LIMITS = dict(side=2048, lights=8)            # csrc/kernels.h's kSceneMaxSide / kSceneMaxLights


def scene_launches(reset=False):
    """``a3vt_scene_render`` calls accepted and kernels launched since the last reset (a test hook, as ``voxel_launches``)."""
    return _launch_counts("a3vt_scene_launches", ("calls", "kernels"), reset)


def _host_table(t, name, dtype, shape):
    """A small HOST table of ``a3vt_scene_render`` (a sequence, an array or a CPU tensor) as a contiguous NumPy array."""
    if isinstance(t, torch.Tensor):
        if t.is_cuda:
            raise RuntimeError(f"a3vt: scene_render reads `{name}` on the host (it is checked there and travels in the launch's "
                               "arguments): pass a sequence, an array or a CPU tensor")
        t = t.numpy()
    a = np.ascontiguousarray(np.asarray(t), dtype=dtype)
    if a.ndim != len(shape) or any(want is not None and want != got for want, got in zip(shape, a.shape)):
        raise ValueError(f"a3vt: scene_render wants {name} of shape {shape}, got {a.shape}")
    return a


def scene_render(verts, faces, face_rgb, centres, radii, sphere_rgb, face_offset, sphere_offset, image_scene, cam_pos, cam_rot,
                 yfov=RENDER_DEFAULTS["yfov"], znear=RENDER_DEFAULTS["znear"], zfar=RENDER_DEFAULTS["zfar"],
                 width=RENDER_DEFAULTS["width"], height=RENDER_DEFAULTS["height"], lights=RENDER_DEFAULTS["lights"],
                 ambient=RENDER_DEFAULTS["ambient"], background=RENDER_DEFAULTS["background"], want_prim=True):
    """Colour, depth and primitive-index images of I views over M scenes of triangles and spheres (``a3vt_scene_render``,
    csrc/scene_render.hip: one launch per 128 images on the current stream, no host synchronisation).  Ray casting with Lambert
    shading under the given lights: NOT pyrender's shader, and never compared with it.

    Device tensors: ``verts`` (V, 3) float32, ``faces`` (F, 3) int32 with global indices, ``face_rgb`` (F, 3) uint8, ``centres``
    (S, 3) and ``radii`` (S,) float32, ``sphere_rgb`` (S, 3) uint8, ``cam_pos`` (I, 3) and ``cam_rot`` (I, 3, 3) float32 (the pose
    matrix ``pretty_render.py`` builds; the camera looks down its -z).  Host tables (sequences, arrays or CPU tensors):
    ``face_offset`` and ``sphere_offset`` (M + 1,), ``image_scene`` (I,), ``lights`` (L, 4) position and intensity, L <= 8,
    ``background`` (3,).  Returns ``{"rgb": (I, H, W, 3) uint8, "depth": (I, H, W) float32, 0 without a hit}`` and, with
    ``want_prim``, ``"prim"`` (I, H, W) int32: the face's index, F + the sphere's index, or -1.  The whole contract is in
    ``include/a3vt.h``."""
    verts, faces, face_rgb = _req(verts, "verts"), _req(faces, "faces", torch.int32), _req(face_rgb, "face_rgb", torch.uint8)
    centres, radii, sphere_rgb = _req(centres, "centres"), _req(radii, "radii"), _req(sphere_rgb, "sphere_rgb", torch.uint8)
    cam_pos, cam_rot = _req(cam_pos, "cam_pos"), _req(cam_rot, "cam_rot")
    I, F, S = cam_pos.shape[0], faces.shape[0], centres.shape[0]
    if cam_pos.shape != (I, 3) or cam_rot.shape != (I, 3, 3) or I < 1:
        raise ValueError(f"a3vt: scene_render wants cam_pos (I, 3) and cam_rot (I, 3, 3), I >= 1, got {tuple(cam_pos.shape)} and "
                         f"{tuple(cam_rot.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.shape != (F, 3) or face_rgb.shape != (F, 3):
        raise ValueError(f"a3vt: scene_render wants verts (V, 3), faces (F, 3) and face_rgb (F, 3), got {tuple(verts.shape)}, "
                         f"{tuple(faces.shape)} and {tuple(face_rgb.shape)}")
    if centres.shape != (S, 3) or radii.shape != (S,) or sphere_rgb.shape != (S, 3):
        raise ValueError(f"a3vt: scene_render wants centres (S, 3), radii (S,) and sphere_rgb (S, 3), got {tuple(centres.shape)}, "
                         f"{tuple(radii.shape)} and {tuple(sphere_rgb.shape)}")
    face_offset = _host_table(face_offset, "face_offset", np.int32, (None,))
    M = len(face_offset) - 1
    if M < 1:
        raise ValueError("a3vt: scene_render wants face_offset (M + 1,), M >= 1")
    sphere_offset = _host_table(sphere_offset, "sphere_offset", np.int32, (M + 1,))
    image_scene = _host_table(image_scene, "image_scene", np.int32, (I,))
    lights = _host_table(np.zeros((0, 4)) if len(lights) == 0 else lights, "lights", np.float32, (None, 4))
    background = _host_table(background, "background", np.uint8, (3,))
    W, H = int(width), int(height)
    if not (1 <= W <= SCENE_LIMITS["side"] and 1 <= H <= SCENE_LIMITS["side"]):      # (before the outputs are sized by them)
        raise RuntimeError(f"a3vt: scene_render: W={W} H={H} outside 1..{SCENE_LIMITS['side']}")
    dev = cam_pos.device
    rgb = torch.empty((I, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((I, H, W), dtype=torch.float32, device=dev)
    prim = torch.empty((I, H, W), dtype=torch.int32, device=dev) if want_prim else None
    host = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    _lib.check(_lib.load().a3vt_scene_render(
        _lib.ptr(verts) if verts.shape[0] else None, verts.shape[0], _lib.ptr(faces) if F else None, _lib.ptr(face_rgb) if F else None, F,
        _lib.ptr(centres) if S else None, _lib.ptr(radii) if S else None, _lib.ptr(sphere_rgb) if S else None, S, host(face_offset),
        host(sphere_offset), M, host(image_scene), _lib.ptr(cam_pos), _lib.ptr(cam_rot), I, float(yfov), float(znear), float(zfar), W, H,
        host(lights), len(lights), float(ambient), host(background), _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(prim), _stream()),
        "scene_render")
    out = {"rgb": rgb, "depth": depth}
    if prim is not None:
        out["prim"] = prim
    return out


POSED_LIMITS = dict(parts=96, instances=1 << 24)    # csrc/kernels.h's kPosedMaxParts / kPosedMaxInstances


def posed_launches(reset=False):
    """``a3vt_scene_render_posed`` calls accepted, the kernels they launched and the kernels of ``a3vt_pose_parts`` since the last
    reset (a test hook, as ``scene_launches``)."""
    return _launch_counts("a3vt_posed_launches", ("calls", "kernels", "pose_parts"), reset)


class PartTable:
    """The template parts of ``scene_render_posed`` / ``pose_parts``: ``parts`` is a sequence of ``(verts (n, 3), faces (m, 3))``
    HOST arrays, the faces with indices into their own part's vertices.  Holds ``verts`` (PV, 3) float32 and ``faces`` (PF, 3) int32
    (made global) on ``device`` (None: the current GPU; "cpu" keeps them on the host, for ``pose_parts``' NumPy form), and on the
    host ``vert_offset`` / ``face_offset`` (P + 1,) int32 and ``bound`` (P, 4) float32: per part the middle of the finite vertices'
    bounds and the largest distance to one, computed in float64 against the float32 centre and rounded UP to float32 (a part
    without a finite vertex gets a zero sphere: none of its faces can be hit).  A face index outside its part's vertices is refused."""

    def __init__(self, parts, device=None):
        parts = [(np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)) for v, f in parts]
        if not 1 <= len(parts) <= POSED_LIMITS["parts"]:
            raise ValueError(f"a3vt: PartTable holds 1..{POSED_LIMITS['parts']} parts (they travel in the launch's arguments), got {len(parts)}")
        verts, faces, bound, base = [], [], np.zeros((len(parts), 4), np.float32), 0
        for p, (v, f) in enumerate(parts):
            if len(f) and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"a3vt: PartTable: part {p} has face indices outside its {len(v)} vertices")
            verts.append(v)
            faces.append(f + base)
            base += len(v)
            good = v[np.isfinite(v).all(axis=1)].astype(np.float64)
            if len(good):
                centre = ((good.min(axis=0) + good.max(axis=0)) / 2).astype(np.float32)
                radius = np.sqrt(((good - centre.astype(np.float64)) ** 2).sum(axis=1).max()) * (1 + 2.0 ** -50)
                r32 = np.float32(radius)
                bound[p, :3], bound[p, 3] = centre, r32 if float(r32) >= radius else np.nextafter(r32, np.float32(np.inf))
        self.num_parts = len(parts)
        self.vert_offset = np.cumsum([0] + [len(v) for v, _ in parts]).astype(np.int32)
        self.face_offset = np.cumsum([0] + [len(f) for _, f in parts]).astype(np.int32)
        self.bound = bound
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.verts = torch.from_numpy(np.concatenate(verts).astype(np.float32).reshape(-1, 3)).to(device)
        self.faces = torch.from_numpy(np.concatenate(faces).astype(np.int32).reshape(-1, 3)).to(device)


def _posed_instances(table, inst_part, inst_pos, inst_rot, inst_rgb, who, cuda):
    if not isinstance(table, PartTable):
        raise ValueError(f"a3vt: {who} wants an ops.PartTable")
    if cuda:
        inst_part, inst_rgb = _req(inst_part, "inst_part", torch.int32), _req(inst_rgb, "inst_rgb", torch.uint8)
        inst_pos, inst_rot = _req(inst_pos, "inst_pos"), _req(inst_rot, "inst_rot")
        _req(table.verts, "table.verts"), _req(table.faces, "table.faces", torch.int32)
    N = inst_part.shape[0]
    if inst_part.shape != (N,) or inst_pos.shape != (N, 3) or inst_rot.shape != (N, 3, 3) or inst_rgb.shape != (N, 3):
        raise ValueError(f"a3vt: {who} wants inst_part (N,), inst_pos (N, 3), inst_rot (N, 3, 3) and inst_rgb (N, 3), got "
                         f"{tuple(inst_part.shape)}, {tuple(inst_pos.shape)}, {tuple(inst_rot.shape)} and {tuple(inst_rgb.shape)}")
    return inst_part, inst_pos, inst_rot, inst_rgb, N


def scene_render_posed(table, inst_part, inst_pos, inst_rot, inst_rgb, inst_offset, cam_pos, cam_rot, yfov=VISION_DEFAULTS["yfov"],
                       znear=VISION_DEFAULTS["znear"], zfar=VISION_DEFAULTS["zfar"], width=VISION_DEFAULTS["width"],
                       height=VISION_DEFAULTS["height"], lights=VISION_DEFAULTS["lights"], ambient=VISION_DEFAULTS["ambient"],
                       background=VISION_DEFAULTS["background"], want_prim=True):
    """Colour, depth and primitive images of I views over scenes of posed INSTANCES of ``table``'s parts
    (``a3vt_scene_render_posed``, csrc/posed_render.hip: one launch per 128 images on the current stream, no workspace, no host
    synchronisation).  ``scene_render``'s ray caster and Lambert shading — NOT pyrender's shader, never compared with it, no alpha.

    Device tensors: ``inst_part`` (N,) int32, ``inst_pos`` (N, 3) and ``inst_rot`` (N, 3, 3) float32, ``inst_rgb`` (N, 3) uint8,
    ``cam_pos`` (I, 3), ``cam_rot`` (I, 3, 3).  Host tables: ``inst_offset`` (I + 1,) — image i owns the instances
    ``inst_offset[i] .. inst_offset[i + 1] - 1`` —, ``lights``, ``background``.  A vertex v of an instance becomes
    ``fma(R[r][0], v.x, fma(R[r][1], v.y, fma(R[r][2], v.z, p[r])))`` per row; from there the rule is ``scene_render``'s, so ``rgb``
    and ``depth`` equal ``scene_render`` on ``pose_parts``' output bit for bit.  An instance with a part id outside the table or a
    non-finite pose is skipped.  Returns ``{"rgb", "depth"}`` and, with ``want_prim``, ``"prim_inst"`` (the instance's index) and
    ``"prim_face"`` (the face's index into ``table.faces``), both -1 without a hit.  The whole contract is in ``include/a3vt.h``."""
    inst_part, inst_pos, inst_rot, inst_rgb, N = _posed_instances(table, inst_part, inst_pos, inst_rot, inst_rgb, "scene_render_posed", True)
    cam_pos, cam_rot = _req(cam_pos, "cam_pos"), _req(cam_rot, "cam_rot")
    I = cam_pos.shape[0]
    if cam_pos.shape != (I, 3) or cam_rot.shape != (I, 3, 3) or I < 1:
        raise ValueError(f"a3vt: scene_render_posed wants cam_pos (I, 3) and cam_rot (I, 3, 3), I >= 1, got {tuple(cam_pos.shape)} and "
                         f"{tuple(cam_rot.shape)}")
    inst_offset = _host_table(inst_offset, "inst_offset", np.int32, (I + 1,))
    lights = _host_table(np.zeros((0, 4)) if len(lights) == 0 else lights, "lights", np.float32, (None, 4))
    background = _host_table(background, "background", np.uint8, (3,))
    W, H = int(width), int(height)
    if not (1 <= W <= SCENE_LIMITS["side"] and 1 <= H <= SCENE_LIMITS["side"]):      # (before the outputs are sized by them)
        raise RuntimeError(f"a3vt: scene_render_posed: W={W} H={H} outside 1..{SCENE_LIMITS['side']}")
    dev = cam_pos.device
    rgb = torch.empty((I, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((I, H, W), dtype=torch.float32, device=dev)
    prim_inst = torch.empty((I, H, W), dtype=torch.int32, device=dev) if want_prim else None
    prim_face = torch.empty((I, H, W), dtype=torch.int32, device=dev) if want_prim else None
    host = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    PV, PF = table.verts.shape[0], table.faces.shape[0]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_scene_render_posed(
            _lib.ptr(table.verts) if PV else None, PV, _lib.ptr(table.faces) if PF else None, PF, host(table.face_offset), host(table.bound),
            table.num_parts, *((_lib.ptr(t) if N else None) for t in (inst_part, inst_pos, inst_rot, inst_rgb)), N, host(inst_offset),
            _lib.ptr(cam_pos), _lib.ptr(cam_rot), I, float(yfov), float(znear), float(zfar), W, H, host(lights), len(lights), float(ambient),
            host(background), _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(prim_inst), _lib.ptr(prim_face), _stream()), "scene_render_posed")
    out = {"rgb": rgb, "depth": depth}
    if want_prim:
        out["prim_inst"], out["prim_face"] = prim_inst, prim_face
    return out


def pose_parts(table, inst_part, inst_pos, inst_rot, inst_rgb, inst_offset=None):
    """The instances of ``scene_render_posed`` written out as triangles (``a3vt_pose_parts``, one launch): instance by instance, the
    part's vertices posed by the kernel's own device function, its faces re-based onto them, the instance's colour per face.
    Returns ``verts`` (TV, 3), ``faces`` (TF, 3) int32, ``face_rgb`` (TF, 3) uint8 — what ``scene_render`` takes — and on the host
    ``vert_base`` / ``face_base`` (N + 1,): instance n owns the rows ``base[n] .. base[n + 1] - 1``, so its face ``f`` of
    ``table.faces`` is row ``face_base[n] + f - table.face_offset[part]``; with ``inst_offset`` (I + 1,) also ``face_offset``
    (I + 1,), the images' face ranges.  An instance with a part id outside the table owns no rows.  ``inst_part`` is read on the
    host to size the output: this call synchronises, unlike the renderer.

    CPU tensors take the same rule in NumPy, each fma as a float64 product and sum rounded to float32 once — which may differ from
    the device's single rounding in the last bit (double rounding)."""
    cuda = isinstance(inst_pos, torch.Tensor) and inst_pos.is_cuda
    inst_part, inst_pos, inst_rot, inst_rgb, N = _posed_instances(table, inst_part, inst_pos, inst_rot, inst_rgb, "pose_parts", cuda)
    part = inst_part.cpu().numpy().astype(np.int64)
    known = (part >= 0) & (part < table.num_parts)
    safe = np.where(known, part, 0)
    vert_base = np.concatenate([[0], np.cumsum(np.where(known, np.diff(table.vert_offset)[safe], 0))]).astype(np.int64)
    face_base = np.concatenate([[0], np.cumsum(np.where(known, np.diff(table.face_offset)[safe], 0))]).astype(np.int64)
    TV, TF = int(vert_base[-1]), int(face_base[-1])
    if max(TV, TF) > 1 << 28:
        raise ValueError(f"a3vt: pose_parts: {TV} vertices / {TF} faces are more than the {1 << 28} of one table")
    out = {"vert_base": vert_base.astype(np.int32), "face_base": face_base.astype(np.int32)}
    if inst_offset is not None:
        out["face_offset"] = face_base[np.asarray(_host_table(inst_offset, "inst_offset", np.int32, (None,)), np.int64)].astype(np.int32)
    if not cuda:
        pv, pf = table.verts.cpu().numpy(), table.faces.cpu().numpy()
        pos, rot, rgb = inst_pos.numpy().astype(np.float64), inst_rot.numpy().astype(np.float64), inst_rgb.numpy()
        verts, faces, face_rgb = np.zeros((TV, 3), np.float32), np.zeros((TF, 3), np.int32), np.zeros((TF, 3), np.uint8)
        fma = lambda a, b, c: (a * b + c).astype(np.float32).astype(np.float64)  # noqa: E731
        for n in np.flatnonzero(known):
            v0, v1 = table.vert_offset[part[n]], table.vert_offset[part[n] + 1]
            f0, f1 = table.face_offset[part[n]], table.face_offset[part[n] + 1]
            v = pv[v0:v1].astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                for r in range(3):
                    verts[vert_base[n]:vert_base[n + 1], r] = fma(rot[n, r, 0], v[:, 0], fma(rot[n, r, 1], v[:, 1],
                                                                                             fma(rot[n, r, 2], v[:, 2], pos[n, r])))
            local = pf[f0:f1].astype(np.int64) - v0
            faces[face_base[n]:face_base[n + 1]] = np.where((local >= 0) & (local < v1 - v0), local + vert_base[n], -1)
            face_rgb[face_base[n]:face_base[n + 1]] = rgb[n]
        return dict(out, verts=torch.from_numpy(verts), faces=torch.from_numpy(faces), face_rgb=torch.from_numpy(face_rgb))
    dev = inst_pos.device
    verts = torch.empty((TV, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((TF, 3), dtype=torch.int32, device=dev)
    face_rgb = torch.empty((TF, 3), dtype=torch.uint8, device=dev)
    vb, fb = torch.from_numpy(out["vert_base"]).to(dev), torch.from_numpy(out["face_base"]).to(dev)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    PV, PF = table.verts.shape[0], table.faces.shape[0]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_pose_parts(
            _lib.ptr(table.verts) if PV else None, PV, _lib.ptr(table.faces) if PF else None, PF, host(table.vert_offset),
            host(table.face_offset), table.num_parts, *((_lib.ptr(t) if N else None) for t in (inst_part, inst_pos, inst_rot, inst_rgb)),
            N, _lib.ptr(vb) if N else None, _lib.ptr(fb) if N else None, _lib.ptr(verts) if TV else None, TV,
            _lib.ptr(faces) if TF else None, _lib.ptr(face_rgb) if TF else None, TF, _stream()), "pose_parts")
    return dict(out, verts=verts, faces=faces, face_rgb=face_rgb)


# csrc/kernels.h's kVoxelMinDim / kVoxelMaxDim / kVoxelMaxMeshes / kVoxelMaxCells / kVoxelMaxDepth
VOXEL_LIMITS = dict(min_dim=4, max_dim=256, meshes=4096, cells=1 << 30, depth=12)


def voxel_launches(reset=False):
    """Operations ``a3vt_voxel_surface`` / ``a3vt_voxel_depth_maps`` / ``a3vt_voxel_points`` enqueued since the last reset (a test
    hook, as ``policy_launches``)."""
    return _launch_counts("a3vt_voxel_launches", ("surface", "depth_maps", "points"), reset)


def _voxel_check(verts, faces, vert_offset, face_offset, dim):
    for t, name, dtype in ((verts, "verts", torch.float32), (faces, "faces", torch.int32), (vert_offset, "vert_offset", torch.int32),
                           (face_offset, "face_offset", torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise RuntimeError(f"a3vt: voxel_surface `{name}` must be a {dtype} tensor")
        if t.device != verts.device:
            raise RuntimeError(f"a3vt: voxel_surface `{name}` is on {t.device}, verts on {verts.device}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"a3vt: voxel_surface wants verts (V, 3) and faces (F, 3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if vert_offset.dim() != 1 or vert_offset.numel() < 2 or face_offset.shape != vert_offset.shape:
        raise ValueError(f"a3vt: voxel_surface wants vert_offset and face_offset (M + 1,), M >= 1, got {tuple(vert_offset.shape)} and "
                         f"{tuple(face_offset.shape)}")
    M, dim, lim = vert_offset.numel() - 1, int(dim), VOXEL_LIMITS
    if not (lim["min_dim"] <= dim <= lim["max_dim"] and M <= lim["meshes"] and M * dim ** 3 <= lim["cells"]):
        raise ValueError(f"a3vt: voxel_surface M={M} dim={dim} outside {lim}")
    return M, dim


def _voxel_mark_host(verts, faces, dim):
    """One mesh's occupancy on NumPy, level by level: the contract of ``a3vt_voxel_surface``'s marking in ``include/a3vt.h``."""
    f32 = np.float32
    grid = np.zeros((dim, dim, dim), dtype=np.uint8)
    finite = verts[np.isfinite(verts)]
    faces = faces[((faces >= 0) & (faces < verts.shape[0])).all(axis=1)]
    if finite.size == 0 or faces.shape[0] == 0:
        return grid
    lo, hi = finite.min(), finite.max()
    with np.errstate(all="ignore"):
        norm = (verts - lo) / (hi - lo) - f32(0.5)
    a, b, c = norm[faces[:, 0]], norm[faces[:, 1]], norm[faces[:, 2]]
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    a, b, c = a[ok], b[ok], c[ok]
    thr = f32((1.0 / dim) ** 2)

    def mark(p):
        f = (p + f32(0.5)) * f32(dim - 1)
        inside = ((f >= 0) & (f < f32(dim))).all(axis=1)
        i = f[inside].astype(np.int64)
        grid[i[:, 0], i[:, 1], i[:, 2]] = 1

    def side(p, q):
        d = p - q
        d = d * d
        return (d[:, 0] + d[:, 1]) + d[:, 2]

    mark(np.concatenate((a, b, c)))
    for _ in range(VOXEL_LIMITS["depth"]):
        split = np.maximum(np.maximum(side(a, b), side(b, c)), side(c, a)) > thr
        if not split.any():
            break
        a, b, c = a[split], b[split], c[split]
        ac, ab, bc = (a + c) * f32(0.5), (a + b) * f32(0.5), (b + c) * f32(0.5)
        mark(np.concatenate((ac, ab, bc)))
        a, b, c = np.concatenate((a, ab, ab, ac)), np.concatenate((ac, b, ac, c)), np.concatenate((ab, bc, bc, bc))
    return grid


def _voxel_depth_maps_host(grid):
    """``extract_ODMs``' values of one (dim, dim, dim) grid, int32 (6, dim, dim)."""
    dim, occ = grid.shape[0], grid != 0
    odm = np.empty((6, dim, dim), dtype=np.int32)
    for axis in range(3):                                  # columns along k, j, i: the maps over (i, j), (i, k), (j, k)
        along = np.moveaxis(occ, 2 - axis, 2)
        some = along.any(axis=2)
        odm[2 * axis] = np.where(some, np.argmax(along[:, :, ::-1], axis=2), dim)      # dim - 1 - last
        odm[2 * axis + 1] = np.where(some, np.argmax(along, axis=2), dim)              # first
    return odm


def _voxel_carve_host(odm):
    """Kept = inside all three column intervals (``apply_ODMs`` with its fill), uint8 (dim, dim, dim)."""
    dim = odm.shape[1]
    x = np.arange(dim)
    i, j, k = x[:, None, None], x[None, :, None], x[None, None, :]
    kept = (k >= odm[1][:, :, None]) & (k <= dim - 1 - odm[0][:, :, None])
    kept &= (j >= odm[3][:, None, :]) & (j <= dim - 1 - odm[2][:, None, :])
    kept &= (i >= odm[5][None, :, :]) & (i <= dim - 1 - odm[4][None, :, :])
    return kept.astype(np.uint8)


def _voxel_surface_host(kept):
    """Surface voxels of a kept grid in lexicographic order, int32 (n, 3)."""
    box = np.pad(kept.astype(np.int32), 1)
    for axis in range(3):                                  # the 3 x 3 x 3 box sum, one axis at a time
        lo = [slice(None)] * 3
        mid, hi = list(lo), list(lo)
        lo[axis], mid[axis], hi[axis] = slice(0, -2), slice(1, -1), slice(2, None)
        box = box[tuple(lo)] + box[tuple(mid)] + box[tuple(hi)]
    return np.argwhere((kept != 0) & (box < 27)).astype(np.int32)


def _voxel_realign_host(surface, verts):
    """``realign_points`` of one mesh's surface rows, fp32 (n, 3), in the reference's order of operations."""
    f32 = np.float32
    out = np.zeros(surface.shape, dtype=f32)
    if surface.shape[0] == 0:
        return out
    for axis in range(3):
        col, x = verts[:, axis], surface[:, axis].astype(f32)
        col = col[np.isfinite(col)]
        hi, lo = x.max(), x.min()
        mid = (hi + lo) * f32(0.5)
        c = x - mid
        p_range = ((hi - mid) + f32(1)) - (lo - mid)
        with np.errstate(all="ignore"):
            v_range = col.max() - col.min() if col.size else f32(np.nan)
            out[:, axis] = (c * v_range) / p_range
    return out


class VoxelSurface:
    """What ``voxel_surface`` returns and ``voxel_points`` consumes: ``counts`` (M,) int32 on the inputs' device, ``occupancy`` /
    ``depth_maps`` when asked for.  On the GPU the tables of the call live in the library's workspace until the next
    ``voxel_surface`` call on that device; on the CPU they are kept here."""

    def __init__(self, M, dim, device, counts, occupancy, depth_maps, host=None):
        self.M, self.dim, self.device, self.counts, self.occupancy, self.depth_maps, self._host = M, dim, device, counts, occupancy, \
            depth_maps, host


def voxel_surface(verts, faces, vert_offset, face_offset, dim, want_occupancy=False, want_depth_maps=False):
    """Voxelise, depth maps, carve and surface count of M meshes (``a3vt_voxel_surface``, csrc/voxel.hip; the whole contract is in
    ``include/a3vt.h``).  ``verts`` (V, 3) float32 and ``faces`` (F, 3) int32 with indices local to each mesh, both concatenated
    over the meshes; ``vert_offset`` / ``face_offset`` (M + 1,) int32.  Returns a ``VoxelSurface``.  GPU tensors run the kernels
    (a fixed number of launches, no host synchronisation); CPU tensors take the same contract on NumPy, with identical results."""
    M, dim = _voxel_check(verts, faces, vert_offset, face_offset, dim)
    dev = verts.device
    if not verts.is_cuda:
        v, f, vo, fo = verts.numpy(), faces.numpy(), vert_offset.numpy(), face_offset.numpy()
        V, F = v.shape[0], f.shape[0]
        host = []
        for m in range(M):
            v0 = min(max(int(vo[m]), 0), V)
            f0 = min(max(int(fo[m]), 0), F)
            vm, fm = v[v0:min(max(int(vo[m + 1]), v0), V)], f[f0:min(max(int(fo[m + 1]), f0), F)]
            occ = _voxel_mark_host(vm, fm, dim)
            odm = _voxel_depth_maps_host(occ)
            host.append((vm, occ, odm, _voxel_surface_host(_voxel_carve_host(odm))))
        counts = torch.tensor([h[3].shape[0] for h in host], dtype=torch.int32)
        occupancy = torch.from_numpy(np.stack([h[1] for h in host])) if want_occupancy else None
        depth_maps = torch.from_numpy(np.stack([h[2] for h in host])) if want_depth_maps else None
        return VoxelSurface(M, dim, dev, counts, occupancy, depth_maps, host)
    verts, faces, vert_offset, face_offset = verts.contiguous(), faces.contiguous(), vert_offset.contiguous(), face_offset.contiguous()
    counts = torch.empty(M, dtype=torch.int32, device=dev)
    occupancy = torch.empty((M, dim, dim, dim), dtype=torch.uint8, device=dev) if want_occupancy else None
    depth_maps = torch.empty((M, 6, dim, dim), dtype=torch.int32, device=dev) if want_depth_maps else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_voxel_surface(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(vert_offset),
                                                  _lib.ptr(face_offset), M, dim, _lib.ptr(occupancy), _lib.ptr(depth_maps),
                                                  _lib.ptr(counts), _stream()), "voxel_surface")
    return VoxelSurface(M, dim, dev, counts, occupancy, depth_maps)


def voxel_points(state, counts=None, index=None, want_aligned=False):
    """The clouds of the ``voxel_surface`` call that returned ``state`` (``a3vt_voxel_points``; no other ``voxel_surface`` call on that
    device may lie between the two).  ``counts``: ``state.counts`` as the caller read it to the host (a list of M ints; read here
    when None — the pipeline's one host read).  ``index`` (M, num_points) int64, or None: row p of mesh m's cloud is its realigned
    surface row ``index[m, p] % n_m``.  Returns a dict: ``surface`` (total, 3) int32, the meshes' surface voxels one after the other,
    each in lexicographic order; ``offset`` (a list of M + 1 ints into it); with ``want_aligned`` ``aligned`` (total, 3) float32;
    with ``index`` ``cloud`` (M, num_points, 3) float32, zeros for a mesh without a surface."""
    M, dim, dev = state.M, state.dim, state.device
    counts = [int(c) for c in (state.counts.tolist() if counts is None else counts)]
    offset = [0]
    for c in counts:
        offset.append(offset[-1] + c)
    total = offset[-1]
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 2 or index.shape[0] != M or \
                index.shape[1] < 1 or index.device != dev:
            raise ValueError(f"a3vt: voxel_points wants index ({M}, num_points >= 1) int64 on {dev}")
        index = index.contiguous()
    out = {"offset": offset}
    if state._host is not None:
        surface = np.concatenate([h[3] for h in state._host]) if M else np.zeros((0, 3), np.int32)
        aligned = [_voxel_realign_host(h[3], h[0]) for h in state._host]
        out["surface"] = torch.from_numpy(surface)
        if want_aligned:
            out["aligned"] = torch.from_numpy(np.concatenate(aligned))
        if index is not None:
            idx = index.numpy()
            cloud = np.zeros((M, idx.shape[1], 3), dtype=np.float32)
            for m in range(M):
                if counts[m]:
                    cloud[m] = aligned[m][idx[m] % counts[m]]
            out["cloud"] = torch.from_numpy(cloud)
        return out
    surface = torch.empty((total, 3), dtype=torch.int32, device=dev)
    aligned = torch.empty((total, 3), dtype=torch.float32, device=dev) if want_aligned else None
    cloud = torch.empty((M, index.shape[1], 3), dtype=torch.float32, device=dev) if index is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().a3vt_voxel_points(M, dim, total, _lib.ptr(surface), _lib.ptr(aligned), _lib.ptr(index),
                                                 index.shape[1] if index is not None else 0, _lib.ptr(cloud), _stream()), "voxel_points")
    out["surface"] = surface
    if want_aligned:
        out["aligned"] = aligned
    if index is not None:
        out["cloud"] = cloud
    return out


def voxel_depth_maps(voxels):
    """``extract_ODMs``' six orthographic depth maps of grids (M, dim, dim, dim) uint8, non-zero = occupied -> (M, 6, dim, dim) int32
    (``a3vt_voxel_depth_maps``: one launch; CPU tensors on NumPy).  The layout is in ``include/a3vt.h``."""
    if not isinstance(voxels, torch.Tensor) or voxels.dtype != torch.uint8 or voxels.dim() != 4 or voxels.shape[1] != voxels.shape[2] or \
            voxels.shape[2] != voxels.shape[3] or voxels.shape[0] < 1:
        raise ValueError("a3vt: voxel_depth_maps wants grids (M, dim, dim, dim) uint8, M >= 1")
    M, dim = voxels.shape[0], voxels.shape[1]
    if not voxels.is_cuda:
        return torch.from_numpy(np.stack([_voxel_depth_maps_host(g) for g in voxels.numpy()]))
    voxels = voxels.contiguous()
    odm = torch.empty((M, 6, dim, dim), dtype=torch.int32, device=voxels.device)
    with torch.cuda.device(voxels.device):
        _lib.check(_lib.load().a3vt_voxel_depth_maps(_lib.ptr(voxels), M, dim, _lib.ptr(odm), _stream()), "voxel_depth_maps")
    return odm


# csrc/kernels.h's kPolicyMaxRows / kPolicyMaxWidth / kPolicyMaxLayers (a3vt_latent_policy_limit returns the library's own): rows
# of a call (and steps of the loss), every layer's in and out, layers of a table.
LATENT_POLICY_MAX = dict(rows=4096, width=1024, layers=16)


def policy_launches(reset=False):
    """Kernel launches of ``a3vt_latent_policy_fwd`` / ``a3vt_action_value_loss`` / ``a3vt_latent_policy_bwd`` since the last
    reset (a test hook, as ``path_counts``)."""
    return _launch_counts("a3vt_latent_policy_launches", ("fwd", "loss", "bwd"), reset)


class PolicyTable:
    """The layer table of ``latent_policy``: ``layers`` = [(weight (out, in), bias (out,), relu), ..] in evaluation order, the
    input of layer ``concat_at`` being cat(previous output, latent, first_latent); ``transform`` None (the last layer's output as
    it is) or ``(scale, offset)`` for ``sigmoid(z) * scale - offset``.  The tensors are used in place; ``struct()`` is the
    ``a3vt_mlp`` of their current addresses."""

    def __init__(self, layers, concat_at, transform=None):
        self.layers = [(w, b, bool(r)) for w, b, r in layers]
        self.concat_at = int(concat_at)
        self.transform = None if transform is None else (float(transform[0]), float(transform[1]))
        if not self.layers:
            raise RuntimeError("a3vt: latent_policy wants at least one layer")
        for l, (w, b, _) in enumerate(self.layers):
            if not (isinstance(w, torch.Tensor) and isinstance(b, torch.Tensor) and w.dim() == 2 and b.shape == (w.shape[0],)):
                raise RuntimeError(f"a3vt: latent_policy layer {l} wants weight (out, in) and bias (out,)")
        if not 1 <= self.concat_at < len(self.layers):
            raise RuntimeError(f"a3vt: latent_policy concat_at={self.concat_at} outside 1..{len(self.layers) - 1}")
        extra = self.layers[self.concat_at][0].shape[1] - self.layers[self.concat_at - 1][0].shape[0]
        if extra < 2 or extra % 2:
            raise RuntimeError(f"a3vt: latent_policy layer {self.concat_at} takes {extra} columns beside the previous output, not 2 * latent_size")
        self.latent_size = extra // 2
        for l in range(1, len(self.layers)):
            want = self.layers[l - 1][0].shape[0] + (extra if l == self.concat_at else 0)
            if self.layers[l][0].shape[1] != want:
                raise RuntimeError(f"a3vt: latent_policy layer {l} in={self.layers[l][0].shape[1]} does not chain (the rows before it give {want})")
        self.in_width, self.num_actions = self.layers[0][0].shape[1], self.layers[-1][0].shape[0]
        self.stash_floats = sum(w.shape[0] for w, _, _ in self.layers)
        self._key, self._struct = None, None

    def params(self):
        return [t for w, b, _ in self.layers for t in (w, b)]

    def in_limits(self):
        """Whether the kernels take this table: fp32 contiguous parameters on one GPU, sizes inside ``LATENT_POLICY_MAX``,
        weight rows on 16-byte boundaries where the kernel loads them so."""
        lim = LATENT_POLICY_MAX
        dev = self.layers[0][0].device
        if len(self.layers) > lim["layers"] or len(self.layers) < 2 or 3 * self.latent_size > lim["width"]:
            return False
        for w, b, _ in self.layers:
            if not (w.is_cuda and w.device == dev and b.device == dev and w.dtype == torch.float32 and b.dtype == torch.float32
                    and w.is_contiguous() and b.is_contiguous() and max(w.shape) <= lim["width"]
                    and w.data_ptr() % (16 if w.shape[1] % 4 == 0 else 4) == 0):
                return False
        return True

    def struct(self):
        key = tuple(t.data_ptr() for t in self.params())
        if key != self._key:
            m = _lib.Mlp()
            for l, (w, b, relu) in enumerate(self.layers):
                m.layer[l] = _lib.MlpLayer(w.data_ptr(), b.data_ptr(), w.shape[1], w.shape[0], 1 if relu else 0, 0)
            m.n_layers, m.concat_at, m.latent_size = len(self.layers), self.concat_at, self.latent_size
            m.transform = 0 if self.transform is None else 1
            m.scale, m.offset = self.transform or (1.0, 0.0)
            self._key, self._struct = key, m
        return self._struct


def _policy_inputs(table, mask, latent, first_latent, taken):
    """Shapes and dtypes of a ``latent_policy`` call (both forms) -> E."""
    for t, name in ((mask, "mask"), (latent, "latent"), (first_latent, "first_latent"), (taken, "taken")):
        if t is None and name == "taken":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
            raise RuntimeError(f"a3vt: latent_policy `{name}` must be a 2-d torch.float32 tensor")
        if t.device != mask.device:
            raise RuntimeError(f"a3vt: latent_policy `{name}` is on {t.device}, the mask on {mask.device}")
    E = mask.shape[0]
    if mask.shape != (E, table.in_width) or latent.shape != (E, table.latent_size) or first_latent.shape != (E, table.latent_size):
        raise RuntimeError(f"a3vt: latent_policy wants mask ({E}, {table.in_width}) and latents ({E}, {table.latent_size}), got "
                           f"{tuple(mask.shape)}, {tuple(latent.shape)}, {tuple(first_latent.shape)}")
    if taken is not None and taken.shape != (E, table.num_actions):
        raise RuntimeError(f"a3vt: latent_policy taken must be ({E}, {table.num_actions}), got {tuple(taken.shape)}")
    if E < 1:
        raise RuntimeError("a3vt: latent_policy rows=0")
    return E


def policy_supported(table, mask):
    """Whether ``latent_policy`` runs the kernels for these operands (else the torch form of the same contract runs)."""
    return bool(mask.is_cuda and table.in_limits() and table.layers[0][0].device == mask.device
                and 1 <= mask.shape[0] <= LATENT_POLICY_MAX["rows"])


def choose_action_torch(values, taken):
    """The action choice of ``a3vt_latent_policy_fwd`` on torch ops: per row the lowest value among ``taken == 0``, a tie to
    the lower index, NaN after +inf, -1 when nothing is open -> (E,) int32."""
    order = torch.sort(values.detach(), dim=1, stable=True).indices       # (ascending, NaN last, equal values keep their order)
    ok = (taken == 0).gather(1, order)
    first = ok.int().argmax(dim=1, keepdim=True)
    chosen = order.gather(1, first).squeeze(1).to(torch.int32)
    return torch.where(ok.any(dim=1), chosen, torch.full_like(chosen, -1))


def _latent_policy_torch(table, mask, latent, first_latent, taken):
    """The contract of ``a3vt_latent_policy_fwd`` on torch ops (CPU tensors, tables outside the kernel's limits)."""
    _policy_inputs(table, mask, latent, first_latent, taken)
    x = mask
    for l, (w, b, relu) in enumerate(table.layers):
        if l == table.concat_at:
            x = torch.cat((x, latent, first_latent), dim=-1)
        x = torch.nn.functional.linear(x, w, b)
        if relu:
            x = torch.relu(x)
    if table.transform is not None:
        x = torch.sigmoid(x) * table.transform[0] - table.transform[1]
    return x, (None if taken is None else choose_action_torch(x, taken))


def latent_policy_fwd(table, mask, latent, first_latent, taken=None, stash=False):
    """One ``a3vt_latent_policy_fwd`` launch, outside autograd -> (values (E, A), action (E,) int32 or None, stash or None)."""
    E = _policy_inputs(table, mask, latent, first_latent, taken)
    L = _lib.load()
    mask, latent, first_latent = _req(mask, "mask"), _req(latent, "latent"), _req(first_latent, "first_latent")
    taken = None if taken is None else _req(taken, "taken")
    dev = mask.device
    values = torch.empty((E, table.num_actions), dtype=torch.float32, device=dev)
    action = None if taken is None else torch.empty(E, dtype=torch.int32, device=dev)
    kept = torch.empty((E, table.stash_floats), dtype=torch.float32, device=dev) if stash else None
    _lib.check(L.a3vt_latent_policy_fwd(ctypes.byref(table.struct()), _lib.ptr(mask), _lib.ptr(latent), _lib.ptr(first_latent),
                                        _lib.ptr(taken), E, _lib.ptr(values), _lib.ptr(action), _lib.ptr(kept), _stream()),
               "latent_policy_fwd")
    return values, action, kept


def latent_policy_bwd(table, mask, latent, first_latent, dvalues, stash, grads, accumulate):
    """The two ``a3vt_latent_policy_bwd`` launches: ``grads`` = [(dweight, dbias), ..] per layer, written (``accumulate`` False)
    or added to (True) in place."""
    E = _policy_inputs(table, mask, latent, first_latent, None)
    L = _lib.load()
    mask, latent, first_latent = _req(mask, "mask"), _req(latent, "latent"), _req(first_latent, "first_latent")
    dvalues, stash = _req(dvalues, "dvalues"), _req(stash, "stash")
    if dvalues.shape != (E, table.num_actions) or stash.shape != (E, table.stash_floats) or len(grads) != len(table.layers):
        raise RuntimeError("a3vt: latent_policy_bwd operand shapes disagree")
    g = _lib.MlpGrads()
    for l, ((dw, db), (w, b, _)) in enumerate(zip(grads, table.layers)):
        dw, db = _req(dw, "dweight"), _req(db, "dbias")
        if dw.shape != w.shape or db.shape != b.shape or dw.data_ptr() != grads[l][0].data_ptr() or db.data_ptr() != grads[l][1].data_ptr():
            raise RuntimeError(f"a3vt: latent_policy_bwd gradient {l} must be contiguous and of its parameter's shape")
        g.dweight[l], g.dbias[l] = dw.data_ptr(), db.data_ptr()
    delta = workspace("latent_policy_delta", E * table.stash_floats * 4, mask.device)
    _lib.check(L.a3vt_latent_policy_bwd(ctypes.byref(table.struct()), ctypes.byref(g), _lib.ptr(mask), _lib.ptr(latent),
                                        _lib.ptr(first_latent), _lib.ptr(dvalues), _lib.ptr(stash), _lib.ptr(delta), E,
                                        1 if accumulate else 0, _stream()), "latent_policy_bwd")


class LatentPolicyFn(torch.autograd.Function):
    """``latent_policy`` under autograd: the forward launch keeps the stash, the backward's two launches write fresh gradient
    tensors (accumulate off).  Only the parameters carry gradients."""

    @staticmethod
    def forward(ctx, table, mask, latent, first_latent, taken, need_bwd, *params):
        values, action, kept = latent_policy_fwd(table, mask, latent, first_latent, taken, stash=need_bwd)
        if need_bwd:
            ctx.table = table
            ctx.save_for_backward(mask, latent, first_latent, kept)
        if action is None:
            action = torch.empty(0, dtype=torch.int32, device=values.device)
        ctx.mark_non_differentiable(action)
        return values, action

    @staticmethod
    def backward(ctx, dvalues, _daction):
        mask, latent, first_latent, kept = ctx.saved_tensors
        table = ctx.table
        grads = [(torch.empty_like(w), torch.empty_like(b)) for w, b, _ in table.layers]
        latent_policy_bwd(table, mask, latent, first_latent, dvalues.contiguous(), kept, grads, accumulate=False)
        return (None,) * 6 + tuple(t for pair in grads for t in pair)


def latent_policy(table, mask, latent, first_latent, taken=None):
    """The value network of the supervised policy (reference ``policies/supervised/model.py:46-58`` and the masking loop of
    ``train.py:119-128``) -> ``(values (E, A), action (E,) int32 or None)``: ``table`` (a ``PolicyTable``) applied to ``mask``
    (E, in), the concat with ``latent`` / ``first_latent`` (E, latent_size), the output transform; with ``taken`` (E, A) also the
    index of the lowest value among ``taken == 0`` (tie: lower index; NaN after +inf; -1 when none is open).  GPU operands inside
    ``LATENT_POLICY_MAX`` run ``a3vt_latent_policy_fwd`` (csrc/latent_policy.hip: one launch; under autograd the backward is two);
    everything else takes the same contract on torch ops.  There are no gradients for mask, latent or first_latent."""
    if not policy_supported(table, mask):
        return _latent_policy_torch(table, mask, latent, first_latent, taken)
    params = table.params()
    values, action = LatentPolicyFn.apply(table, mask, latent, first_latent, taken, _wants_grad(*params), *params)
    return values, (None if taken is None else action)


def _action_value_check(values, actions, targets):
    """Shapes, dtypes and the action range of ``action_value_loss`` (both forms) -> (actions on the values' device, T, E, A).
    ``actions`` on the host (a NumPy array or a CPU tensor) are checked there; on the GPU the check costs a host sync."""
    if isinstance(actions, np.ndarray):
        actions = torch.from_numpy(np.ascontiguousarray(actions))
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2:
        raise RuntimeError("a3vt: action_value_loss `values` must be a 2-d torch.float32 tensor")
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.float32 or targets.device != values.device:
        raise RuntimeError("a3vt: action_value_loss `targets` must be a torch.float32 tensor on the values' device")
    if not isinstance(actions, torch.Tensor) or actions.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("a3vt: action_value_loss `actions` must be an int32 / int64 tensor or array")
    E, A = values.shape
    if actions.dim() != 2 or actions.shape[1] != E or targets.shape != actions.shape or actions.shape[0] < 1 or E < 1:
        raise RuntimeError(f"a3vt: action_value_loss wants actions and targets (T, {E}), got {tuple(actions.shape)} and {tuple(targets.shape)}")
    if bool(((actions < 0) | (actions >= A)).any()):
        raise RuntimeError(f"a3vt: action_value_loss actions outside [0, {A})")
    lim = LATENT_POLICY_MAX
    if actions.shape[0] > lim["rows"] or E > lim["rows"] or A > lim["width"]:
        raise RuntimeError(f"a3vt: action_value_loss steps={actions.shape[0]} rows={E} num_actions={A} outside {lim}")
    return actions.to(values.device, torch.int32).contiguous(), actions.shape[0], E, A


def _action_value_loss_torch(values, actions, targets):
    """The contract of ``a3vt_action_value_loss`` on torch ops -> (loss, dvalues); ``loss`` carries autograd."""
    actions, T, E, A = _action_value_check(values, actions, targets)
    idx = actions.long()
    pred = values.gather(1, idx.t()).t()                                     # (T, E): values[e][actions[t][e]]
    loss = ((targets - pred) ** 2).mean()
    with torch.no_grad():
        dvalues = torch.zeros_like(values)
        for t in range(T):                                                   # (repeated pairs add up in t order)
            dvalues.scatter_add_(1, idx[t].unsqueeze(1), ((pred[t] - targets[t]) * (2.0 / (T * E))).unsqueeze(1))
    return loss, dvalues


class ActionValueLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, actions, targets):
        L = _lib.load()
        T, E = actions.shape
        values, targets = _req(values, "values"), _req(targets, "targets")
        loss = torch.empty((), dtype=torch.float32, device=values.device)
        dvalues = torch.empty_like(values)
        _lib.check(L.a3vt_action_value_loss(_lib.ptr(values), _lib.ptr(actions), _lib.ptr(targets), T, E, values.shape[1], _lib.ptr(loss),
                                            _lib.ptr(dvalues), _stream()), "action_value_loss")
        ctx.save_for_backward(dvalues)
        ctx.mark_non_differentiable(dvalues)
        return loss, dvalues

    @staticmethod
    def backward(ctx, gloss, _gd):
        (dvalues,) = ctx.saved_tensors
        return gloss * dvalues, None, None


def action_value_loss(values, actions, targets):
    """The supervised trainer's loss (reference ``policies/supervised/train.py:148-155``) -> ``(loss, dvalues)``:
    ``loss = mean_{t,e} (targets[t][e] - values[e][actions[t][e]])^2`` for ``values`` (E, A), ``actions`` (T, E) integers and
    ``targets`` (T, E), and ``dvalues`` (E, A) its gradient, repeated (e, a) pairs added in t order.  An action outside [0, A) is
    refused (checked on the host: hand ``actions`` over as a NumPy array or CPU tensor to keep the device queue running).
    GPU values run ``a3vt_action_value_loss`` (one launch); CPU values take the same contract on torch ops.  ``loss`` carries
    autograd towards ``values``."""
    if not values.is_cuda:
        return _action_value_loss_torch(values, actions, targets)
    actions, T, E, A = _action_value_check(values, actions, targets)
    return ActionValueLossFn.apply(values, actions, targets)


# ---- DDQN's Latent_Model on the layer table (csrc/ddqn_latent.hip) -----------------------------------------------------------

def ddqn_latent_launches(reset=False):
    """Kernel launches of ``a3vt_ddqn_latent_q`` / ``a3vt_ddqn_latent_update`` since the last reset (a test hook)."""
    return _launch_counts("a3vt_ddqn_latent_launches", ("q", "update"), reset)


def ddqn_latent_supported(table, mask):
    """Whether the two ``ddqn_latent`` ops run the kernels for these operands (else the torch form of the same contract runs):
    what ``policy_supported`` asks, no output transform, the mask as wide as the action table, A <= 304."""
    return bool(policy_supported(table, mask) and table.transform is None and table.in_width == table.num_actions
                and table.num_actions <= LATENT_NN_MAX["num_actions"])


def _ddqn_latent_q_torch(table, mask, latent, first_latent, mask_penalty):
    q, _ = _latent_policy_torch(table, mask, latent, first_latent, None)
    if mask_penalty is None:
        return q, None
    return q, q.detach().masked_fill(mask_penalty > 0, -1e10).max(1)[1].to(torch.int32)


def ddqn_latent_q(table, mask, latent, first_latent, mask_penalty=None):
    """DDQN's ``Latent_Model`` -> ``(q (E, A), action (E,) int32 or None)``: ``q`` unpenalised; with ``mask_penalty`` (E, A) also
    ``argmax(mask_penalty > 0 ? -1e10 : q)``, the lowest index on a tie (index 0 when every action is taken).  No autograd.  GPU
    operands inside the limits run ``a3vt_ddqn_latent_q`` (one launch; ``q`` has the bits of ``latent_policy_fwd``'s values);
    everything else takes the same contract on torch ops."""
    if mask_penalty is not None and (mask_penalty.dtype != torch.float32 or mask_penalty.shape != (mask.shape[0], table.num_actions)
                                     or mask_penalty.device != mask.device):
        raise RuntimeError(f"a3vt: ddqn_latent_q mask_penalty must be a float32 ({mask.shape[0]}, {table.num_actions}) tensor on the mask's device")
    if not ddqn_latent_supported(table, mask):
        with torch.no_grad():
            return _ddqn_latent_q_torch(table, mask, latent, first_latent, mask_penalty)
    E = _policy_inputs(table, mask, latent, first_latent, None)
    L = _lib.load()
    mask, latent, first_latent = _req(mask, "mask"), _req(latent, "latent"), _req(first_latent, "first_latent")
    pen = None if mask_penalty is None else _req(mask_penalty, "mask_penalty")
    q = torch.empty((E, table.num_actions), dtype=torch.float32, device=mask.device)
    action = None if pen is None else torch.empty(E, dtype=torch.int32, device=mask.device)
    _lib.check(L.a3vt_ddqn_latent_q(ctypes.byref(table.struct()), _lib.ptr(mask), _lib.ptr(latent), _lib.ptr(first_latent), _lib.ptr(pen), E,
                                    _lib.ptr(q), _lib.ptr(action), _stream()), "ddqn_latent_q")
    return q, action


def _ddqn_latent_update_torch(online, target, grads, mask, mask_n, latent, latent_n, first_latent, actions, rewards, denom, budget, gamma):
    """The contract of ``a3vt_ddqn_latent_update`` composed from the torch forms of the existing ops."""
    params = [p.detach().requires_grad_(True) for p in online.params()]
    live = PolicyTable([(params[2 * l], params[2 * l + 1], r) for l, (_, _, r) in enumerate(online.layers)], online.concat_at, online.transform)
    q_cur, _ = _latent_policy_torch(live, mask, latent, first_latent, None)
    with torch.no_grad():
        q_no, _ = _latent_policy_torch(online, mask_n, latent_n, first_latent, None)
        q_nt, _ = _latent_policy_torch(target, mask_n, latent_n, first_latent, None)
    loss, best, tgt = _ddqn_td_torch(q_cur, q_no, q_nt, mask, actions, rewards, denom, budget, gamma)
    got = torch.autograd.grad(loss, params)
    with torch.no_grad():
        for l, (dw, db) in enumerate(grads):
            dw.copy_(got[2 * l])
            db.copy_(got[2 * l + 1])
        act = actions.long().clamp(0, q_cur.shape[1] - 1)
        diff = q_cur.detach().gather(1, act.unsqueeze(1)).squeeze(1) - tgt
    return loss.detach(), q_cur.detach(), best, tgt, diff


def ddqn_latent_update(online, target, grads, mask, mask_n, latent, latent_n, first_latent, actions, rewards, denom, budget, gamma):
    """The device work of one double-DQN update of a ``Latent_Model`` (reference ``policies/DDQN/ddqn.py:81-115`` and the backward)
    -> ``(loss, q_cur (B, A), best_next int32 (B,), target (B,), diff (B,))``; ``grads`` = [(dweight, dbias), ..] per layer of
    ``online`` are OVERWRITTEN with the loss gradient.  ``online`` / ``target``: two ``PolicyTable`` of the same sizes, no transform.
    No autograd.  GPU operands inside the limits run ``a3vt_ddqn_latent_update``: three launches, no host sync, every output with
    the bits of ``latent_policy_fwd`` x 3, ``ddqn_td``, its backward under a unit gradient and ``latent_policy_bwd(accumulate=False)``.
    Everything else takes the same contract on torch ops."""
    B = _policy_inputs(online, mask, latent, first_latent, None)
    _policy_inputs(online, mask_n, latent_n, first_latent, None)
    if [(tuple(w.shape), r) for w, _, r in online.layers] != [(tuple(w.shape), r) for w, _, r in target.layers] or \
            online.concat_at != target.concat_at:
        raise RuntimeError("a3vt: ddqn_latent_update wants an online and a target table of the same layers")
    for t, name in ((actions, "actions"), (rewards, "rewards"), (denom, "denom")):
        if t is None and name == "denom":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != (B,) or t.device != mask.device:
            raise RuntimeError(f"a3vt: ddqn_latent_update `{name}` must be a float32 ({B},) tensor on the mask's device")
    if len(grads) != len(online.layers):
        raise RuntimeError("a3vt: ddqn_latent_update wants one (dweight, dbias) pair per layer")
    for l, ((dw, db), (w, b, _)) in enumerate(zip(grads, online.layers)):
        if dw.shape != w.shape or db.shape != b.shape or dw.dtype != torch.float32 or db.dtype != torch.float32 or \
                not (dw.is_contiguous() and db.is_contiguous()) or dw.device != w.device or db.device != b.device:
            raise RuntimeError(f"a3vt: ddqn_latent_update gradient {l} must be contiguous float32 and of its parameter's shape and device")
    if not (ddqn_latent_supported(online, mask) and target.in_limits() and target.layers[0][0].device == mask.device
            and target.transform is None and B <= LATENT_POLICY_MAX["rows"]):
        return _ddqn_latent_update_torch(online, target, grads, mask, mask_n, latent, latent_n, first_latent, actions, rewards, denom,
                                         budget, gamma)
    L = _lib.load()
    mask, mask_n, latent, latent_n, first_latent = (_req(t, n) for t, n in ((mask, "mask"), (mask_n, "mask_n"), (latent, "latent"),
                                                                            (latent_n, "latent_n"), (first_latent, "first_latent")))
    actions, rewards = _req(actions, "actions"), _req(rewards, "rewards")
    denom = None if denom is None else _req(denom, "denom")
    g = _lib.MlpGrads()
    for l, (dw, db) in enumerate(grads):
        g.dweight[l], g.dbias[l] = dw.data_ptr(), db.data_ptr()
    dev, A = mask.device, online.num_actions
    q_cur = torch.empty((B, A), dtype=torch.float32, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    tgt, diff = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    scratch = workspace("ddqn_latent", B * (2 * A + 2 * online.stash_floats) * 4, dev)
    _lib.check(L.a3vt_ddqn_latent_update(ctypes.byref(online.struct()), ctypes.byref(target.struct()), ctypes.byref(g), _lib.ptr(mask),
                                         _lib.ptr(mask_n), _lib.ptr(latent), _lib.ptr(latent_n), _lib.ptr(first_latent),
                                         _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(denom), B, int(budget), float(gamma),
                                         _lib.ptr(q_cur), _lib.ptr(best), _lib.ptr(tgt), _lib.ptr(diff), _lib.ptr(loss),
                                         _lib.ptr(scratch), _stream()), "ddqn_latent_update")
    return loss, q_cur, best, tgt, diff


class QnetInputFn(torch.autograd.Function):
    """Features + layer 0 of the DDQN graph model on ``a3vt_qnet_input_fwd/bwd`` (csrc/qnet_input.hip).  ``mesh`` (B, N, 4);
    the composites ``comp_s`` (B, npad), ``comp_t`` (4, npad), ``comp_c`` (50, npad) come padded to npad = pad4(h) columns."""

    @staticmethod
    def forward(ctx, mesh, w1, b1, w2, b2, comp_s, comp_t, comp_c, bias, adj, cut_len, need_bwd):
        L = _lib.load()
        mesh, w1, b1, w2, b2, comp_s, comp_t, comp_c, bias = (
            _req(t, n) for t, n in ((mesh, "mesh"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (comp_s, "comp_s"),
                                    (comp_t, "comp_t"), (comp_c, "comp_c"), (bias, "bias")))
        B, N, _ = mesh.shape
        h = bias.shape[0]
        npad = (h + 3) // 4 * 4
        if N != adj.n:
            raise RuntimeError(f"a3vt: the mesh has {N} vertices but the adjacency has {adj.n}")
        if mesh.shape[2] != 4 or w1.shape != (25, 63) or b1.shape != (25,) or w2.shape != (50, 25) or b2.shape != (50,) or \
                comp_s.shape != (B, npad) or comp_t.shape != (4, npad) or comp_c.shape != (50, npad):
            raise RuntimeError("a3vt: qnet_input operand shapes disagree")
        y = torch.empty((B, N, npad), dtype=torch.float32, device=mesh.device)
        scratch = workspace("qnet", L.a3vt_qnet_input_scratch_bytes(B, N, h, cut_len, 1 if need_bwd else 0), mesh.device)
        _lib.check(L.a3vt_qnet_input_fwd(_lib.ptr(mesh), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(comp_s),
                                         _lib.ptr(comp_t), _lib.ptr(comp_c), _lib.ptr(bias), h, cut_len, _lib.ptr(adj.rowptr),
                                         _lib.ptr(adj.col), _lib.ptr(adj.val), adj.max_degree, N, B, _lib.ptr(y), npad,
                                         _lib.ptr(scratch), _stream()), "qnet_input_fwd")
        ctx.adj, ctx.dims = adj, (h, npad, cut_len)
        ctx.save_for_backward(mesh, w1, b1, w2, b2, comp_c, y)
        return y[..., :h] if npad != h else y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.load()
        mesh, w1, b1, w2, b2, comp_c, y = ctx.saved_tensors
        h, npad, cut_len = ctx.dims
        adj = ctx.adj
        B, N, _ = mesh.shape
        gy = _req(gy, "grad_output")
        dev = mesh.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        d_s, d_t, d_c = new(B, npad), new(4, npad), new(50, npad)
        dw1, db1, dw2, db2, gb = new(25, 63), new(25), new(50, 25), new(50), new(h)
        scratch = workspace("qnet", L.a3vt_qnet_input_scratch_bytes(B, N, h, cut_len, 1), dev)
        _lib.check(L.a3vt_qnet_input_bwd(_lib.ptr(mesh), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(comp_c), h,
                                         cut_len, _lib.ptr(adj.t_rowptr), _lib.ptr(adj.t_col), _lib.ptr(adj.t_val), adj.t_max_degree,
                                         N, B, _lib.ptr(y), npad, _lib.ptr(gy), gy.shape[-1], _lib.ptr(d_s), _lib.ptr(d_t),
                                         _lib.ptr(d_c), _lib.ptr(dw1), _lib.ptr(db1), _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(gb),
                                         _lib.ptr(scratch), _stream()), "qnet_input_bwd")
        return None, dw1, db1, dw2, db2, d_s, d_t, d_c, gb, None, None, None


def qnet_input_supported(hidden):
    return 1 <= hidden <= 304


def qnet_input(mesh, action, pos_enc, mask_table, weight, bias, adj, cut_len):
    """``relu(layer0([action | PE(p) | E[token]]))`` of ``Graph_Model`` without the feature rows: ``mesh`` (B, N, 4) = positions
    and mask tokens, ``action`` (B, 100) the action embedding, ``pos_enc`` the ``Positional_Encoder(100)`` module, ``mask_table``
    (4, 100), ``weight`` (300, h) / ``bias`` (h,) of layer 0 -> (B, N, h).  The composites S = a Wa + b3 Wp, T = E Wm and
    C = W3^T Wp are formed here on torch ops, so autograd carries their gradients to the action model, the table, the encoder's
    last layer and the three row blocks of the weight; the kernel returns the gradients of the encoder's first two layers and of
    the bias.  No position gradient."""
    l1, l2, l3 = pos_enc.model[0], pos_enc.model[2], pos_enc.model[4]
    wa, wp, wm = weight[:100], weight[100:200], weight[200:300]
    comp_s = torch.addmm(l3.bias @ wp, action, wa)
    comp_t = mask_table @ wm
    comp_c = l3.weight.t() @ wp
    pad = (-weight.shape[1]) % 4
    if pad:
        comp_s, comp_t, comp_c = (torch.nn.functional.pad(t, (0, pad)) for t in (comp_s, comp_t, comp_c))
    params = (l1.weight, l1.bias, l2.weight, l2.bias, comp_s, comp_t, comp_c, bias)
    return QnetInputFn.apply(mesh, *params, adj, cut_len, _wants_grad(*params))


def rowgemm(a, w, bf16=False):
    """C = A @ W on the MFMA kernel (tests / bench): a (M,K) with K % 4 == 0, w (K,N) with N <= 304."""
    L = _lib.load()
    a, w = _req(a, "a"), _req(w, "w")
    M, K = a.shape
    N = w.shape[1]
    wt = torch.empty((L.a3vt_wt_rows(N), L.a3vt_wt_ld(K)), dtype=torch.float32, device=a.device)
    _lib.check(L.a3vt_transpose_weight(_lib.ptr(w), K, N, _lib.ptr(wt), _stream()), "transpose_weight")
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.check(L.a3vt_rowgemm(_lib.ptr(a), K, M, K, _lib.ptr(wt), N, 1 if bf16 else 0, _lib.ptr(c), N, _stream()),
               "rowgemm")
    return c


CSR_ALGOS = {"auto": 0, "rows": 1, "sliced": 2}


def dbg_csr_algo(name):
    """Test hook (``a3vt_dbg_csr_algo``): force the neighbour-aggregation kernels of the fp32 stacks — "auto" (default, by
    shape), "rows" (half-wave per vertex) or "sliced" (channel-sliced wherever a mesh slice fits LDS).  Same outputs."""
    _lib.check(_lib.load().a3vt_dbg_csr_algo(CSR_ALGOS[name]), "dbg_csr_algo")


def split3(x):
    """The exact operand split of gemm mode 3 (``a3vt_split3_bf16``): three int16 tensors of bf16 bit patterns with
    ``hi + mid + lo == x``."""
    L = _lib.load()
    x = _req(x, "x")
    hi, mid, lo = (torch.empty(x.shape, dtype=torch.int16, device=x.device) for _ in range(3))
    _lib.check(L.a3vt_split3_bf16(_lib.ptr(x), x.numel(), _lib.ptr(hi), _lib.ptr(mid), _lib.ptr(lo), _stream()), "split3_bf16")
    return hi, mid, lo


def check_finite(t, flag):
    """Deferred NaN/Inf check: ORs 1 into `flag` (int32 device scalar) without syncing the host."""
    L = _lib.load()
    _lib.check(L.a3vt_check_finite(_lib.ptr(t), t.numel(), _lib.ptr(flag), _stream()), "check_finite")
