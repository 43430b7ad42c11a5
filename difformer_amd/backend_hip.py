"""Tensor-level wrapper of the C ABI: allocation (torch caching allocator), stream plumbing
(torch's current HIP stream) and layout checks.  No arithmetic happens here.

Every method requires float32 tensors resident on a ROCm device and raises otherwise --
the package has no CPU or eager path.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from .sliced import SlicedPlan
from .tensor_cache import MISS, TensorCache


def _ptr(t):
    """Device address as a plain int (None = NULL): ctypes converts it for `c_void_p` argtypes itself, and a Python int is
    several times cheaper to make than a c_void_p object -- the host path has ~20 of these per call."""
    return t.data_ptr() if t is not None else None


# Part 0 of the row-sharded SpMM runs while the all-gather of the value rows is in flight.  A workgroup of the blocked
# kernel owns a whole CU, so it is launched on fewer workgroups than the 256 CUs and the collective's kernel keeps CUs
# of its own (RCCL uses up to ~32 channels = workgroups).
PART0_WORKGROUPS = int(os.environ.get("DIFFORMER_SPMM_PART0_WGS", "224"))

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev):
    """Raw handle of torch's current HIP stream on `dev` (the fast accessor when this torch has it)."""
    if _raw_stream is not None and dev.index is not None:
        return _raw_stream(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


def _require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "difformer_amd: operands must live on the MI355X (got a CPU tensor); this package has no "
                "CPU fallback -- move the model and inputs to the GPU with .to('cuda')")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"difformer_amd: operands on different devices ({dev} vs {t.device})")
    return dev


def _f32(t, name):
    if t.dtype != torch.float32:
        raise TypeError(f"difformer_amd: {name} must be float32 (got {t.dtype}); the reference path is fp32 "
                        "(difformer.py:27)")
    return t


def _all_f32(**named):
    """Every operand that is given (not None) must be float32; the keyword is the name in the message."""
    for name, t in named.items():
        if t is not None and t.dtype != torch.float32:
            _f32(t, name)


_SUFFIX = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _storage(*tensors):
    """Common storage dtype of the operands -> C-ABI suffix ('f32' | 'bf16')."""
    dt = None
    for t in tensors:
        if t is None:
            continue
        if t.dtype not in _SUFFIX:
            raise TypeError(f"difformer_amd: unsupported dtype {t.dtype}: float32 (reference dtype) or bfloat16 "
                            "(storage-only variant) expected")
        if dt is None:
            dt = t.dtype
        elif t.dtype != dt:
            raise TypeError(f"difformer_amd: operands mix {dt} and {t.dtype}")
    return dt, _SUFFIX[dt]


def _row_major(t, width):
    """Return (tensor, leading dimension in elements) with the trailing dims dense so that
    row r starts at data_ptr + r*ld*4 and holds `width` contiguous floats.  Strided row views
    (e.g. column slices of a fused projection) are passed through without a copy."""
    ok = t.stride(-1) == 1 or t.shape[-1] == 1
    if ok and t.dim() == 3:
        ok = t.stride(1) == t.shape[2] or t.shape[1] == 1
    if ok and t.shape[0] > 1:
        ok = t.stride(0) >= width
    if not ok:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else width
    return t, int(ld)


def _rows(t, width, align=False):
    """_row_major of an optional operand: None -> (None, 0).  align: the kernel reads the rows four elements at a time,
    so a leading dimension that is no multiple of 4 elements, or a first row that does not start on a 4-element
    boundary, is replaced by a dense copy."""
    if t is None:
        return None, 0
    t, ld = _row_major(t, width)
    if align and (ld % 4 or t.data_ptr() % (4 * t.element_size())):
        # dense rows that merely start off the boundary (a slice of a flat buffer) are contiguous already: clone them
        return (t.clone() if t.is_contiguous() else t.contiguous()), width
    return t, ld


def _contig(*tensors, f32=None):
    """The operands made contiguous, None staying None; f32: the name under which each must also be float32."""
    if f32 is not None:
        for t in tensors:
            if t is not None and t.dtype != torch.float32:
                _f32(t, f32)
    return [None if t is None else t.contiguous() for t in tensors]


def _workspace(nbytes, dev, floor=0, or_none=False):
    """Scratch bytes of one call.  floor: allocate at least that much (the kernel is handed an address even when it asks
    for nothing); or_none: no buffer at all when the kernel asks for nothing."""
    if or_none and not nbytes:
        return None
    return torch.empty(max(nbytes, floor), dtype=torch.uint8, device=dev)


def _loss_rows(t, C):
    """[n, C] operand of a loss kernel -> (tensor, leading dimension in elements).  Rows of unit column stride at least C
    apart are taken as they are, aligned to their element only; anything else (a column step, overlapping rows) is copied."""
    n = t.shape[0]
    if (t.stride(1) != 1 and C > 1) or (n > 1 and t.stride(0) < C):
        t = t.contiguous()
    return t, (int(t.stride(0)) if n > 1 else C)


def _slice_major(F, plan, dev):
    """ys [F/4, T*NT, 4]: the slice-major copy of [n, F] rows that sliced_spmm reads (plan: sliced_plan's geometry)."""
    return torch.empty((F // 4, plan.T * plan.NT, 4), dtype=torch.float32, device=dev)


def _check_edge_index(edge_index):
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise TypeError("difformer_amd: edge_index must be an int64 tensor of shape [2, E]")


def _kept_status(dev):
    """int64 [2] = [kept count | status word] that a filtering kernel fills -> (both, count, status): ONE read-back."""
    res = torch.zeros(2, dtype=torch.int64, device=dev)
    return res, res[:1], res[1:].view(torch.int32)


def _read_kept(res, ids, num_nodes):
    """Kept count of _kept_status after the call; raises when the status word reports node ids (`ids`) out of range."""
    kept, bad = res.tolist()                                # one sync: the result size is data dependent
    if bad & 0xFFFFFFFF:
        raise IndexError(f"difformer_amd: {ids} node ids outside [0, {num_nodes})")
    return kept


def _edge_operands(q, k, scale):
    """Operands of the edge-attention entry points (include/difformer_edges.h): q [N,H,M], k [L,H,M] float32 as aligned rows
    (views that are not are copied), scale [N,H] float32 dense or None -> (device, leading arguments, tensors to keep alive)."""
    dev = _require_device(q, k, scale)
    _all_f32(q=q, k=k, scale=scale)
    N, H, M = q.shape
    q, ldq = _rows(q, H * M, align=True)
    k, ldk = _rows(k, H * M, align=True)
    if scale is not None:
        if tuple(scale.shape) != (N, H):
            raise ValueError(f"difformer_amd: scale must be [N, H] = [{N}, {H}] (got {tuple(scale.shape)})")
        scale = scale.contiguous()
    return dev, (_ptr(q), ldq, _ptr(k), ldk, _ptr(scale), N, k.shape[0], H, M), (q, k, scale)


class _Timed:
    """HIP-event bracket around one C-ABI call (events on the launching stream): the slow path of HipBackend._call."""

    def __init__(self, backend, name, dev):
        only = backend.kernel_events_only          # bracket just these entry points (keeps the host ahead of the GPU)
        self.rec = backend.kernel_events if (only is None or name in only) else None
        self.name, self.dev = name, dev

    def __enter__(self):
        # device guard only when the operands live on another device than the current one
        self.ctx = None
        if self.dev.index is None or torch.cuda.current_device() != self.dev.index:
            self.ctx = torch.cuda.device(self.dev)
            self.ctx.__enter__()
        if self.rec is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record(torch.cuda.current_stream(self.dev))
            self.rec.setdefault(self.name, []).append((self.start, end))
        return self.ctx.__exit__(*exc) if self.ctx is not None else False


class HipBackend:
    has_tiny = True          # the whole-model kernels for tiny graphs (tiny.py; csrc/tiny_model.hip) are in this library
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        # bench.py sets this to a dict to collect (start, end) HIP events per entry point
        self.kernel_events = None
        self.kernel_events_only = None
        self._ones = {}                             # device -> float32 [1] = 1.0 (device-side beta of dif_rowgemm_f32)
        self._packed = TensorCache(64)              # weight tensor, geometry -> its packed copy (_cached_pack)
        self._adam_tickets = {}                     # device -> int32 [DIF_ADAM_MAX_TENSORS], all zero between calls (adam_step)
        from . import ops
        self.lib.dif_set_exact_fp32(1 if ops.EXACT_FP32 else 0)      # a set_exact_fp32 made before the library was loaded

    def set_exact_fp32(self, flag):
        """The launchers' side of ops.set_exact_fp32: which matrix core their products take (dif_set_exact_fp32)."""
        return bool(self.lib.dif_set_exact_fp32(1 if flag else 0))

    def kernel_times_ms(self):
        """{entry point: [ms per call]} from the collected events (synchronises)."""
        torch.cuda.synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in (self.kernel_events or {}).items()}

    def _call(self, label, symbol, dev, *args, maps=False, edges=False, knn=False, slots=False, metrics=False, loss=False,
              adam=False, readout=False, nbr=False):
        """Every launch goes through here: `symbol` of the C ABI with `args` and, last, torch's current stream on `dev`;
        a non-zero return raises DifformerHipError naming the symbol.  `label` is the key of the call's events in
        `kernel_events` (usually a family of symbols: bench.py and the tests key on it).  The common case -- no event
        collection, operands on the current device -- adds nothing around the call.  maps / edges / knn / slots / metrics /
        loss / adam / readout / nbr: `symbol` is one of libdifformer_maps.so (include/difformer_maps.h) / libdifformer_edges.so
        (include/difformer_edges.h) / libdifformer_knn.so (include/difformer_knn.h) / libdifformer_slots.so
        (include/difformer_slots.h) / libdifformer_metrics.so (include/difformer_metrics.h) / libdifformer_loss.so
        (include/difformer_loss.h) / libdifformer_adam.so (include/difformer_adam.h) / libdifformer_readout.so
        (include/difformer_readout.h) / libdifformer_nbr.so (include/difformer_nbr.h), loaded on first use."""
        side = ((_lib.load_maps, _lib.check_maps) if maps else (_lib.load_edges, _lib.check_edges) if edges else
                (_lib.load_knn, _lib.check_knn) if knn else (_lib.load_slots, _lib.check_slots) if slots else
                (_lib.load_metrics, _lib.check_metrics) if metrics else (_lib.load_loss, _lib.check_loss) if loss else
                (_lib.load_adam, _lib.check_adam) if adam else (_lib.load_readout, _lib.check_readout) if readout else
                (_lib.load_nbr, _lib.check_nbr) if nbr else None)
        fn = getattr(side[0]() if side else self.lib, symbol)
        index = dev.index
        if self.kernel_events is None and index is not None and torch.cuda.current_device() == index:
            rc = fn(*args, _raw_stream(index) if _raw_stream is not None else _stream(dev))
        else:
            with _Timed(self, label, dev):
                rc = fn(*args, _stream(dev))
        if rc != 0:
            (side[1] if side else _lib.check)(rc, symbol)

    # ---- a1 --------------------------------------------------------------------------------
    def simple_reduce(self, q, k, v):
        dev = _require_device(q, k, v)
        n, H, M = q.shape
        D = v.shape[2]
        _, sfx = _storage(q, k, v)
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        reduced = torch.empty(self.lib.dif_simple_reduced_len(H, M, D), dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_simple_workspace_bytes(n, H, M, D)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_simple_reduce_f32", "dif_simple_reduce_" + sfx, dev, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv,
                   n, H, M, D, _ptr(reduced), _ptr(ws), ws_bytes)
        return reduced

    def project_reduce(self, x, Wq, bq, Wk, bk, Wv, bv, H, D):
        """x [n,C] -> (q [n,H,D], v [n,H,D], reduced): projections fused with stage 1 of the simple kernel."""
        dev = _require_device(x, Wq, bq, Wk, bk, Wv, bv)
        n, C = x.shape
        dt, sfx = _storage(x, Wq, bq, Wk, bk, Wv, bv)
        x, ldx = _row_major(x, C)
        ws_ = _contig(Wq, bq, Wk, bk, Wv, bv)
        q = torch.empty((n, H, D), dtype=dt, device=dev)
        v = torch.empty((n, H, D), dtype=dt, device=dev)
        reduced = torch.empty(self.lib.dif_simple_reduced_len(H, D, D), dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_project_reduce_workspace_bytes(n, H, D)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_project_reduce_f32", "dif_project_reduce_" + sfx, dev, _ptr(x), ldx, n, C,
                   *[_ptr(t) for t in ws_], H, D, _ptr(q), H * D, _ptr(v), H * D, _ptr(reduced), _ptr(ws), ws_bytes)
        return q, v, reduced

    def simple_apply(self, q, reduced, n_global, D):
        dev = _require_device(q, reduced)
        n, H, M = q.shape
        dt, sfx = _storage(q)
        _f32(reduced, "reduced")
        q, ldq = _row_major(q, H * M)
        out = torch.empty((n, H, D), dtype=dt, device=dev)
        self._call("dif_simple_apply_f32", "dif_simple_apply_" + sfx, dev, _ptr(q), ldq, _ptr(reduced), n,
                   int(n_global), H, M, D, _ptr(out), H * D)
        return out

    # ---- a1 backward ------------------------------------------------------------------------
    def simple_backward(self, q, k, v, reduced, out, g, shard=None):
        """(dq, dk, dv) of the simple kernel for fp32 q,k [n,H,M], v/out/g [n,H,D] with M, D <= 512.  Row-sharded
        (`shard`, `reduced` already summed over the ranks): the sums over nodes of the backward -- q^T gn, sum gn, the
        ks-gradient -- are all-reduced in one buffer, then the scalar T: two small exchange steps."""
        dev = _require_device(q, k, v, reduced, out, g)
        n, H, M = q.shape
        sharded = shard is not None and shard.world > 1
        n_global = shard.n_global if sharded else n
        D = v.shape[2]
        _all_f32(q=q, k=k, v=v, out=out, grad=g)
        # q, k, v are usually column slices of one fused projection [n, 3 H D]: every kernel below takes a leading
        # dimension, so they go in as they are (three 34-MB copies per layer at C4 otherwise)
        (q, ldq), (k, ldk), (v, ldv) = _row_major(q, H * M), _row_major(k, H * M), _row_major(v, H * D)
        out, g = out.contiguous(), g.contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        gn, gd = torch.empty((n, H, D), **f32), torch.empty((n, H), **f32)
        sums = torch.empty(H * M + 1, **f32)
        ws_bytes = self.lib.dif_simple_bwd_workspace_bytes(n, H, M, D)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_simple_bwd_prep_f32", "dif_simple_bwd_prep_f32", dev, _ptr(q), ldq, _ptr(g), H * D, _ptr(out),
                   H * D, _ptr(reduced), n, int(n_global), H, M, D, _ptr(gn), _ptr(gd), _ptr(sums), _ptr(ws), ws_bytes)
        rec2 = self.simple_reduce(q, q, gn)                      # q^T gn, (sum q), sum gn
        if sharded:
            both = torch.cat([rec2, sums])
            shard.all_reduce_sum(both)
            rec2, sums = both[: rec2.numel()], both[rec2.numel():]
        # small per-head coefficient tensors, all on the device (no host synchronisation)
        hmd = H * M * D
        s = torch.rsqrt(reduced[-2]) * torch.rsqrt(reduced[-1])
        ktv_s = (reduced[:hmd] * s).contiguous()                 # s KtV          [H,M,D]
        ks_s = (reduced[hmd:hmd + H * M] * s).contiguous()       # s ks           [H,M]
        dktv = (rec2[:hmd] * s).contiguous()                     # s q^T gn       [H,M,D]
        dvs = rec2[hmd + H * M: hmd + H * M + H * D].contiguous()
        dks = (sums[: H * M] * s).contiguous()
        if M == D and (H * M) % 4 == 0:
            # dq | dk | dv as the column blocks of ONE [n, 3 H D] buffer: when q, k, v were the column slices of a fused
            # projection, the gradient of that projection is this buffer as it stands (autograd_ops._SplitColumns finds the
            # views adjacent and skips its concatenation: 308 MB of copy per layer at 100,000 x 128)
            fused = torch.empty((n, 3 * H * M), **f32)
            fused._difformer_fused_grad = True      # only a buffer made HERE may be completed in place by _SplitColumns
            dq, dk, dv = (fused[:, i * H * M: (i + 1) * H * M].view(n, H, M) for i in range(3))
            ldg = 3 * H * M
        else:
            dq, dk, dv = torch.empty((n, H, M), **f32), torch.empty((n, H, M), **f32), torch.empty((n, H, D), **f32)
            ldg = None

        def rowgemm(A, K, mat, mat_t, bias, r, u, cin, beta, C, dst, lda=None, ldc=None):
            self._call("dif_rowgemm_f32", "dif_rowgemm_f32", dev, _ptr(A), lda or H * K, _ptr(mat), D, M * D, mat_t, 1.0,
                       _ptr(bias), _ptr(r), _ptr(u), 1.0, _ptr(cin), ldc or H * C, _ptr(beta), n, H, K, C, _ptr(dst),
                       ldg or H * C)

        rowgemm(gn, D, ktv_s, 1, None, gd, ks_s, None, None, M, dq)   # dq_main = gn (s KtV)^T + gd (s ks)
        # T = s * dL/ds = sum q . dq_main.  (Algebraically also -(vs . dvs) - N sum gd, but those two terms cancel to
        # ~1e-4 of their size at N ~ 1e5; this form has no cancellation.)
        T = (q * dq).sum()
        if sharded:
            T = shard.all_reduce_sum(T.reshape(1))[0]
        dq.addcmul_(q, (-T / reduced[-2]).expand_as(q))               # - (T/|Q|^2) q
        beta_k = (-T / reduced[-1]).reshape(1).contiguous()
        rowgemm(v, D, dktv, 1, dks, None, None, k, beta_k, M, dk, lda=ldv, ldc=ldk)     # v dKtV^T + dks - (T/|K|^2) k
        rowgemm(k, M, dktv, 0, dvs, None, None, None, None, D, dv, lda=ldk)             # k dKtV + dvs
        return dq, dk, dv

    # ---- a2 --------------------------------------------------------------------------------
    def sigmoid_attention(self, q, k, v, want_den=False):
        """-> out [N,H,D]; want_den (fp32, training): (out, den float32 [N,H]) for sigmoid_backward."""
        dev = _require_device(q, k, v)
        N, H, M = q.shape
        L, D = k.shape[0], v.shape[2]
        dt, sfx = _storage(q, k, v)          # bfloat16: storage only, scores / sigma / sums in fp32
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        out = torch.empty((N, H, D), dtype=dt, device=dev)
        ws_bytes = self.lib.dif_sigmoid_workspace_bytes(N, L, H, M, D)
        ws = _workspace(ws_bytes, dev, or_none=True)
        head = (_ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, N, L, H, M, D, _ptr(out), H * D)
        if want_den:                         # the _fwd_ symbol takes `den` between the output and the workspace
            _f32(q, "q")
            den = torch.empty((N, H), dtype=torch.float32, device=dev)
            self._call("dif_sigmoid_attn_fwd_f32", "dif_sigmoid_attn_fwd_f32", dev, *head, _ptr(den), _ptr(ws), ws_bytes)
            return out, den
        self._call("dif_sigmoid_attn_" + sfx, "dif_sigmoid_attn_" + sfx, dev, *head, _ptr(ws), ws_bytes)
        return out

    # ---- attention maps (libdifformer_maps.so) --------------------------------------------------
    def attn_topk(self, q, k, mode, topk):
        """q [N,H,M], k [L,H,M] float32, M a multiple of 4 up to 512 -> (values float32, indices int32) [N,H,topk]: per
        query row and head the `topk` largest s = q . k over the keys, descending, ties to the lower key (mode 0: value s;
        mode 1: value sigma(s) / sum_l sigma(s)).  The [N, L] scores never exist (csrc/attn_topk.hip)."""
        dev = _require_device(q, k)
        _all_f32(q=q, k=k)
        N, H, M = q.shape
        L = k.shape[0]
        q, ldq = _rows(q, H * M, align=True)
        k, ldk = _rows(k, H * M, align=True)
        maps = _lib.load_maps()
        values = torch.empty((N, H, topk), dtype=torch.float32, device=dev)
        indices = torch.empty((N, H, topk), dtype=torch.int32, device=dev)
        ws_bytes = maps.dif_attn_topk_workspace_bytes(N, L, H, M, topk)
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_attn_topk_f32", "dif_attn_topk_f32", dev, _ptr(q), ldq, _ptr(k), ldk, N, L, H, M, int(mode), int(topk),
                   _ptr(values), _ptr(indices), _ptr(ws), ws_bytes, maps=True)
        return values, indices

    # ---- k-nearest-neighbour graphs (libdifformer_knn.so) -----------------------------------------
    def knn_graph(self, x, k, loop, metric, centre_row, want_dist=False, route=-1):
        """x [N,M] float32, M a multiple of 4 up to 512, 1 <= k <= 24 -> (edge_index int64 [2, N kk], dist float32 [N kk] or
        None), kk = min(k, N - (0 if loop else 1)): per row its kk nearest rows, nearest first, ranked by float64 distances
        (metric 0: squared Euclidean, 1: cosine), ties to the lower index; row `centre_row` of edge_index holds the row
        itself, the other its neighbours.  route: -1 (automatic), 0 (direct, M <= 16), 1 (sweep).  No [N, N] tensor exists
        (csrc/knn_graph.hip).  x is taken as it is: rows of unit column stride that start on 16-byte boundaries (the caller,
        neighbors.py, copies any other view)."""
        dev = _require_device(x)
        _all_f32(x=x)
        N, M = x.shape
        ldx = int(x.stride(0)) if N > 1 else M
        if x.stride(1) != 1 or ldx < M or ldx % 4 or x.data_ptr() % 16:
            raise ValueError("difformer_amd: knn_graph takes rows of unit column stride on 16-byte boundaries "
                             f"(got strides {tuple(x.stride())}, address % 16 = {x.data_ptr() % 16})")
        knn = _lib.load_knn()
        kk = min(int(k), N - (0 if loop else 1))
        edge_index = torch.empty((2, N * kk), dtype=torch.int64, device=dev)
        dist = torch.empty(N * kk, dtype=torch.float32, device=dev) if want_dist else None
        ws_bytes = knn.dif_knn_workspace_bytes(N, M, int(k), int(bool(loop)), int(metric), int(route))
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_knn_graph_f32", "dif_knn_graph_f32", dev, _ptr(x), ldx, N, M, int(k), int(bool(loop)), int(metric),
                   int(centre_row), int(route), _ptr(edge_index), _ptr(dist), _ptr(ws), ws_bytes, knn=True)
        return edge_index, dist

    # ---- neighbour graphs of a batch (libdifformer_nbr.so) -----------------------------------------
    @staticmethod
    def _nbr_operands(who, x, graph_ptr):
        dev = _require_device(x, graph_ptr)
        _all_f32(x=x)
        N, M = x.shape
        ldx = int(x.stride(0)) if N > 1 else M
        if x.stride(1) != 1 or ldx < M or ldx % 4 or x.data_ptr() % 16:
            raise ValueError(f"difformer_amd: {who} takes rows of unit column stride on 16-byte boundaries "
                             f"(got strides {tuple(x.stride())}, address % 16 = {x.data_ptr() % 16})")
        if graph_ptr.dtype != torch.int32 or graph_ptr.dim() != 1 or graph_ptr.shape[0] < 2 or not graph_ptr.is_contiguous():
            raise ValueError(f"difformer_amd: {who} takes graph_ptr as a contiguous int32 [B + 1] (got {graph_ptr.dtype}, "
                             f"{tuple(graph_ptr.shape)})")
        return dev, N, M, ldx, graph_ptr.shape[0] - 1

    def nbr_knn(self, x, graph_ptr, edge_ptr, E, k, loop, metric, centre_row, want_dist=False):
        """x [N,M] float32, M a multiple of 4 up to 64; graph_ptr int32 [B + 1] as ops.BatchLayout makes it; edge_ptr int64
        [B + 1], edge_ptr[b] = sum over b' < b of n_b' kk_b' with kk_b = min(k, n_b - (0 if loop else 1)), edge_ptr[B] == E (the
        caller, neighbors.py, knows E on the host) -> (edge_index int64 [2, E], dist float32 [E] or None): per row its kk_b
        nearest rows of its own graph, nearest first, as `knn_graph` ranks them (csrc/nbr_batched.hip)."""
        dev, N, M, ldx, B = self._nbr_operands("nbr_knn", x, graph_ptr)
        if edge_ptr.dtype != torch.int64 or tuple(edge_ptr.shape) != (B + 1,) or edge_ptr.device != dev or not edge_ptr.is_contiguous():
            raise ValueError(f"difformer_amd: nbr_knn takes edge_ptr as a contiguous int64 [{B + 1}] on {dev}")
        E = int(E)
        edge_index = torch.empty((2, E), dtype=torch.int64, device=dev)
        dist = torch.empty(E, dtype=torch.float32, device=dev) if want_dist else None
        self._call("dif_nbr_knn_f32", "dif_nbr_knn_f32", dev, _ptr(x), ldx, N, M, _ptr(graph_ptr), _ptr(edge_ptr), B, int(k),
                   int(bool(loop)), int(metric), int(centre_row), _ptr(edge_index) if E else None, E,
                   _ptr(dist) if E else None, nbr=True)
        return edge_index, dist

    def nbr_radius_lists(self, x, graph_ptr, r, loop, cap):
        """x, graph_ptr as nbr_knn -> (deg int32 [N], workspace): per row the number of rows of its own graph with squared
        float64 distance < r r (strict; at most `cap`, the nearest kept) and, in the workspace, their ranked lists for
        nbr_radius_edges (csrc/nbr_batched.hip)."""
        dev, N, M, ldx, B = self._nbr_operands("nbr_radius_lists", x, graph_ptr)
        nbr = _lib.load_nbr()
        deg = torch.empty(N, dtype=torch.int32, device=dev)
        ws_bytes = nbr.dif_nbr_workspace_bytes(N, int(cap))
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_nbr_radius_lists_f32", "dif_nbr_radius_lists_f32", dev, _ptr(x), ldx, N, M, _ptr(graph_ptr), B, float(r),
                   int(bool(loop)), int(cap), _ptr(deg), _ptr(ws), ws_bytes, nbr=True)
        return deg, ws

    def nbr_radius_edges(self, deg_ptr, E, cap, centre_row, ws, want_dist=False):
        """deg_ptr int64 [N + 1], the exclusive prefix sum of nbr_radius_lists' deg with deg_ptr[N] == E, and its workspace ->
        (edge_index int64 [2, E], dist float32 [E] or None): centres ascending, nearest first."""
        dev = _require_device(deg_ptr, ws)
        if deg_ptr.dtype != torch.int64 or deg_ptr.dim() != 1 or deg_ptr.shape[0] < 2 or not deg_ptr.is_contiguous():
            raise ValueError("difformer_amd: nbr_radius_edges takes deg_ptr as a contiguous int64 [N + 1]")
        N, E = deg_ptr.shape[0] - 1, int(E)
        edge_index = torch.empty((2, E), dtype=torch.int64, device=dev)
        dist = torch.empty(E, dtype=torch.float32, device=dev) if want_dist else None
        self._call("dif_nbr_radius_edges", "dif_nbr_radius_edges", dev, _ptr(deg_ptr), N, int(cap), int(centre_row), _ptr(ws),
                   ws.numel(), _ptr(edge_index) if E else None, E, _ptr(dist) if E else None, nbr=True)
        return edge_index, dist

    # ---- evaluation metrics (libdifformer_metrics.so) ---------------------------------------------
    def rocauc_counts(self, score, cls):
        """score [n,C] float32 and cls [n,C] uint8 class codes (0 negative, 1 positive, 2 unlabelled, 3 another value), rows of
        unit column stride -> int64 [C,5] = per column {P, N, unlabelled, invalid, U2}: roc_auc_score of a column is
        U2 / (2 P N) (csrc/eval_metrics.hip).  n C <= 2^31 - 1: the caller (metrics.py) cuts the columns into groups."""
        dev = _require_device(score, cls)
        _all_f32(score=score)
        n, C = score.shape
        if cls.dtype != torch.uint8 or tuple(cls.shape) != (n, C):
            raise ValueError(f"difformer_amd: rocauc_counts takes uint8 class codes of shape {(n, C)} (got {cls.dtype}, "
                             f"{tuple(cls.shape)})")
        if score.stride(1) != 1 and C > 1:
            score = score.contiguous()
        if cls.stride(1) != 1 and C > 1:
            cls = cls.contiguous()
        lds = int(score.stride(0)) if n > 1 else C
        ldc = int(cls.stride(0)) if n > 1 else C
        if lds < C:
            score, lds = score.contiguous(), C
        if ldc < C:
            cls, ldc = cls.contiguous(), C
        met = _lib.load_metrics()
        counts = torch.empty((C, 5), dtype=torch.int64, device=dev)
        ws_bytes = met.dif_rocauc_workspace_bytes(n, C)
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_rocauc_counts_f32", "dif_rocauc_counts_f32", dev, _ptr(score), lds, _ptr(cls), ldc, n, C, _ptr(counts),
                   _ptr(ws), ws_bytes, metrics=True)
        return counts

    def argmax_correct(self, pred, label, labelled):
        """pred [n,K] float32 (rows of unit column stride), label int64 [n], labelled uint8 [n] -> int64 [2] = {labelled rows
        whose first maximal index (NaN above every number) equals the label, labelled rows} (csrc/eval_metrics.hip)."""
        dev = _require_device(pred, label, labelled)
        _all_f32(pred=pred)
        n, K = pred.shape
        if label.dtype != torch.int64 or labelled.dtype != torch.uint8 or label.shape != (n,) or labelled.shape != (n,):
            raise ValueError(f"difformer_amd: argmax_correct takes int64 labels and a uint8 mask of shape ({n},)")
        if pred.stride(1) != 1 and K > 1:
            pred = pred.contiguous()
        ldp = int(pred.stride(0)) if n > 1 else K
        if ldp < K:
            pred, ldp = pred.contiguous(), K
        label, labelled = label.contiguous(), labelled.contiguous()
        out = torch.empty(2, dtype=torch.int64, device=dev)
        self._call("dif_argmax_correct_f32", "dif_argmax_correct_f32", dev, _ptr(pred), ldp, _ptr(label), _ptr(labelled), n, K,
                   _ptr(out), metrics=True)
        return out

    # ---- the optimiser update (libdifformer_adam.so) ----------------------------------------------
    def adam_step(self, params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay):
        """One Adam step (csrc/adam.hip; formula and rounding: include/difformer_adam.h) of params[i] under grads[i], in place,
        with the moments exp_avgs[i] / exp_avg_sqs[i] and the float32 0-d step counters steps[i], which the kernel increments.
        Dense float32 tensors on one device, aligned to their element; ceil(len / DIF_ADAM_MAX_TENSORS) launches on the current
        stream, no host synchronisation.  The caller bumps the parameters' version counters."""
        if not params:
            return
        dev = _require_device(*params)
        table = []
        for p, g, m, v, t in zip(params, grads, exp_avgs, exp_avg_sqs, steps, strict=True):
            n = p.numel()
            for name, x in (("param", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v)):
                if x.dtype != torch.float32 or x.device != dev or x.numel() != n or not x.is_contiguous():
                    raise ValueError(f"difformer_amd: adam_step: {name} must be a dense float32 tensor of {n} elements on {dev} "
                                     f"(got {x.dtype}, {tuple(x.shape)}, strides {x.stride()}, {x.device})")
            if t.dtype != torch.float32 or t.device != dev or t.numel() != 1:
                raise ValueError(f"difformer_amd: adam_step: step must be one float32 on {dev} (got {t.dtype}, {tuple(t.shape)}, {t.device})")
            table += (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), n)
        tickets = self._adam_tickets.get(dev)
        if tickets is None:
            tickets = self._adam_tickets[dev] = torch.zeros(_lib.ADAM_CONSTANTS["DIF_ADAM_TICKET_BYTES"] // 4, dtype=torch.int32,
                                                            device=dev)
        rows = (ctypes.c_int64 * len(table))(*table)
        self._call("dif_adam_step_f32", "dif_adam_step_f32", dev, rows, len(params), lr, beta1, beta2, eps, weight_decay,
                   _ptr(tickets), adam=True)

    # ---- training losses (libdifformer_loss.so) ---------------------------------------------------
    def loss_row_weights(self, index, n):
        """int64 index [m] (any order, duplicates count) -> (int32 [n] multiplicity of every row, int32 [1] number of indices
        outside [0, n)); integer atomics only (csrc/loss.hip)."""
        dev = _require_device(index)
        if index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError(f"difformer_amd: loss_row_weights takes a 1-d int64 index (got {index.dtype}, {tuple(index.shape)})")
        index = index.contiguous()
        weight = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        self._call("dif_loss_row_weights", "dif_loss_row_weights", dev, _ptr(index), index.shape[0], n, _ptr(weight), _ptr(status),
                   loss=True)
        return weight, status

    @staticmethod
    def _loss_operands(kind, out, second, rows, ignore_index):
        """The leading arguments the forward and the backward of one loss share: logits [n,C] and, for kind 'nll', int64 labels
        [n], for 'bce' a target [n,C] of int64 / float32 / uint8, both as row-strided views (stride(0) is the leading
        dimension: a column slice is NOT copied); rows None | int32 [n] weights | uint8 [n] mask.
        -> (device, suffix, n, C, arguments up to rows_kind, tensors to keep alive)."""
        dev = _require_device(out, second, rows)
        _, sfx = _storage(out)
        n, C = out.shape
        out, ldx = _loss_rows(out, C)
        const = _lib.LOSS_CONSTANTS
        if rows is None:
            rows_kind = const["DIF_LOSS_ROWS_ALL"]
        elif rows.dtype == torch.int32 and rows.shape == (n,):
            rows, rows_kind = rows.contiguous(), const["DIF_LOSS_ROWS_WEIGHTS"]
        elif rows.dtype == torch.uint8 and rows.shape == (n,):
            rows, rows_kind = rows.contiguous(), const["DIF_LOSS_ROWS_MASK"]
        else:
            raise ValueError(f"difformer_amd: the row selection of a loss is int32 weights or a uint8 mask of shape ({n},) "
                             f"(got {rows.dtype}, {tuple(rows.shape)})")
        if kind == "nll":
            if second.dtype != torch.int64 or second.shape != (n,):
                raise ValueError(f"difformer_amd: the NLL takes int64 labels of shape ({n},) (got {second.dtype}, {tuple(second.shape)})")
            second = second.contiguous()
            args = (_ptr(out), ldx, _ptr(second), int(ignore_index), _ptr(rows), rows_kind)
        else:
            types = {torch.int64: "DIF_LOSS_TARGET_I64", torch.float32: "DIF_LOSS_TARGET_F32", torch.uint8: "DIF_LOSS_TARGET_U8"}
            if second.dtype not in types or tuple(second.shape) != (n, C):
                raise ValueError(f"difformer_amd: the BCE takes an int64, float32 or uint8 target of shape {(n, C)} "
                                 f"(got {second.dtype}, {tuple(second.shape)})")
            second, ldt = _loss_rows(second, C)
            args = (_ptr(out), ldx, _ptr(second), const[types[second.dtype]], ldt, _ptr(rows), rows_kind)
        return dev, sfx, n, C, args, (out, second, rows)

    def loss_forward(self, kind, out, second, rows=None, index_status=None, ignore_index=-100):
        """-> the 32-byte record of include/difformer_loss.h as float64 [4]: [0] the loss, .view(float32)[2] the loss rounded
        to float32, .view(int64)[2] count, .view(int64)[3] invalid.  index_status: loss_row_weights' status word."""
        dev, sfx, n, C, args, keep = self._loss_operands(kind, out, second, rows, ignore_index)
        lib = _lib.load_loss()
        record = torch.empty(4, dtype=torch.float64, device=dev)
        ws_bytes = lib.dif_loss_workspace_bytes(n, C)
        ws = _workspace(ws_bytes, dev, floor=16)
        symbol = ("dif_nll_log_softmax_fwd_" if kind == "nll" else "dif_bce_with_logits_fwd_") + sfx
        self._call(symbol, symbol, dev, *args, _ptr(index_status), n, C, _ptr(record), _ptr(ws), ws_bytes, loss=True)
        return record

    def loss_backward(self, kind, out, second, record, upstream, rows=None, ignore_index=-100):
        """-> d loss / d out [n,C] in out's dtype, every element written (csrc/loss.hip).  upstream: float32 scalar on the device."""
        dev, sfx, n, C, args, keep = self._loss_operands(kind, out, second, rows, ignore_index)
        _require_device(record, upstream)
        if upstream.dtype != torch.float32 or upstream.numel() != 1:
            raise ValueError(f"difformer_amd: the upstream gradient of a loss is one float32 (got {upstream.dtype}, {tuple(upstream.shape)})")
        grad = torch.empty((n, C), dtype=out.dtype, device=dev)
        symbol = ("dif_nll_log_softmax_bwd_" if kind == "nll" else "dif_bce_with_logits_bwd_") + sfx
        self._call(symbol, symbol, dev, *args, n, C, _ptr(record), _ptr(upstream), _ptr(grad), C, loss=True)
        return grad

    # ---- graph read-out (libdifformer_readout.so) --------------------------------------------------
    @staticmethod
    def _readout_table(who, graph_ptr, dev):
        if graph_ptr.dtype != torch.int32 or graph_ptr.dim() != 1 or graph_ptr.shape[0] < 1 or graph_ptr.device != dev:
            raise ValueError(f"difformer_amd: {who} takes graph_ptr as int32 [B + 1] on {dev} (got {graph_ptr.dtype}, "
                             f"{tuple(graph_ptr.shape)}, {graph_ptr.device})")
        return graph_ptr.contiguous()

    def readout_fwd(self, x, graph_ptr, mode):
        """x [N, H] float32 or bfloat16 (a row-strided view is not copied), graph_ptr int32 [B + 1] as ops.BatchLayout makes it
        (graph b = rows [graph_ptr[b], graph_ptr[b+1]), graph_ptr[B] == N), mode 'add' | 'mean' | 'max' -> [B, H] in x's dtype,
        every element written (csrc/graph_readout.hip; arithmetic and edge semantics: include/difformer_readout.h)."""
        dev = _require_device(x, graph_ptr)
        _, sfx = _storage(x)
        N, H = x.shape
        graph_ptr = self._readout_table("readout_fwd", graph_ptr, dev)
        B = graph_ptr.shape[0] - 1
        x, ldx = _loss_rows(x, H)
        out = torch.empty((B, H), dtype=x.dtype, device=dev)
        symbol = "dif_readout_fwd_" + sfx
        self._call(symbol, symbol, dev, _ptr(x), ldx, _ptr(graph_ptr), B, N, H, _lib.READOUT_CONSTANTS["DIF_READOUT_" + mode.upper()],
                   _ptr(out), H, readout=True)
        return out

    def readout_bwd(self, grad_out, graph_ptr, mode, n_rows, x=None, pooled=None):
        """grad_out [B, H] -> d / d x [n_rows, H] in grad_out's dtype, every element written once.  mode 'max' needs the
        forward's x and its result `pooled`; the other modes read neither."""
        dev = _require_device(grad_out, graph_ptr, x, pooled)
        _, sfx = _storage(grad_out, x, pooled)
        B, H = grad_out.shape
        graph_ptr = self._readout_table("readout_bwd", graph_ptr, dev)
        if graph_ptr.shape[0] != B + 1:
            raise ValueError(f"difformer_amd: readout_bwd: grad_out has {B} rows for {graph_ptr.shape[0] - 1} graphs")
        grad_out, ldgo = _loss_rows(grad_out, H)
        ldx = ldp = 0
        if mode == "max":
            if x is None or pooled is None or tuple(x.shape) != (n_rows, H) or tuple(pooled.shape) != (B, H):
                raise ValueError(f"difformer_amd: readout_bwd: mode 'max' needs x {(n_rows, H)} and pooled {(B, H)}")
            x, ldx = _loss_rows(x, H)
            pooled, ldp = _loss_rows(pooled, H)
        else:
            x = pooled = None
        grad_x = torch.empty((n_rows, H), dtype=grad_out.dtype, device=dev)
        symbol = "dif_readout_bwd_" + sfx
        self._call(symbol, symbol, dev, _ptr(x), ldx, _ptr(pooled), ldp, _ptr(grad_out), ldgo, _ptr(graph_ptr), B, n_rows, H,
                   _lib.READOUT_CONSTANTS["DIF_READOUT_" + mode.upper()], _ptr(grad_x), H, readout=True)
        return grad_x

    # ---- attention on graph edges (libdifformer_edges.so) ----------------------------------------
    def edge_attention(self, q, k, scale, edge_index, mode):
        """q [N,H,M], k [L,H,M] float32 (M a multiple of 4 up to 512), scale [N,H] float32 or None, edge_index int64 [2,E]
        (row 0 the key id, row 1 the query id) -> (out float32 [E,H], status int32 [3]): out[e,h] = f(q[col_e,h] . k[row_e,h])
        scale[col_e,h] with f the identity (mode 0) or sigma (mode 1).  An id out of range gives NaN for its edge and
        status = [any, a key id, a query id] != 0; the caller reads it (csrc/attn_edges.hip)."""
        dev, head, keep = _edge_operands(q, k, scale)
        _require_device(q, edge_index)
        _check_edge_index(edge_index)
        ei = edge_index.contiguous()
        E, H = int(ei.shape[1]), q.shape[1]
        out = torch.empty((E, H), dtype=torch.float32, device=dev)
        status = torch.empty(3, dtype=torch.int32, device=dev)
        self._call("dif_edge_attn_f32", "dif_edge_attn_f32", dev, *head, int(mode), _ptr(ei), E, _ptr(out), _ptr(status), edges=True)
        return out, status

    def edge_attention_mass(self, q, k, scale, rowptr, src, mode):
        """Operands as edge_attention; rowptr int32 [>= N + 1], src int32: the target-row CSR of csr_build -> mass float32
        [N,H]: mass[n,h] = scale[n,h] sum_j f(q[n,h] . k[src[j],h]) over row n's entries, in an order that depends on M alone."""
        dev, head, keep = _edge_operands(q, k, scale)
        _require_device(q, rowptr, src)
        N, H = q.shape[0], q.shape[1]
        if rowptr.dtype != torch.int32 or src.dtype != torch.int32 or rowptr.numel() < N + 1:
            raise TypeError("difformer_amd: rowptr (at least N + 1 entries) and src must be int32")
        rowptr, src = rowptr.contiguous(), src.contiguous()
        mass = torch.empty((N, H), dtype=torch.float32, device=dev)
        self._call("dif_edge_attn_mass_f32", "dif_edge_attn_mass_f32", dev, *head, int(mode), _ptr(rowptr), _ptr(src), int(src.numel()),
                   _ptr(mass), edges=True)
        return mass

    def sigmoid_backward(self, q, k, v, out, den, g):
        """(dq, dk, dv) of the sigmoid kernel for fp32 q [N,H,M], k [L,H,M], v [L,H,D], out / g [N,H,D], den [N,H];
        M, D <= 512 (csrc/sigmoid_attn_bwd.hip up to 64 columns, csrc/sigmoid_wide.hip beyond: sigma recomputed tile by tile,
        nothing of size N x L stored)."""
        dev = _require_device(q, k, v, out, den, g)
        N, H, M = q.shape
        L, D = k.shape[0], v.shape[2]
        _all_f32(q=q, k=k, v=v, out=out, den=den, grad=g)
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        g, ldg = _row_major(g, H * D)
        out, den = out.contiguous(), den.contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        dq, dk, dv = torch.empty((N, H, M), **f32), torch.empty((L, H, M), **f32), torch.empty((L, H, D), **f32)
        ws_bytes = self.lib.dif_sigmoid_bwd_workspace_bytes(N, L, H, M, D)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_sigmoid_attn_bwd_f32", "dif_sigmoid_attn_bwd_f32", dev, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv,
                   _ptr(out), H * D, _ptr(den), _ptr(g), ldg, N, L, H, M, D, _ptr(dq), H * M, _ptr(dk), H * M, _ptr(dv),
                   H * D, _ptr(ws), ws_bytes)
        return dq, dk, dv

    # ---- f4: batch of graphs (physical particle/difformer-v2.py:71-137) ---------------------
    def batched_simple_attention(self, q, k, v, graph_ptr, want_den=False):
        """graph_ptr: int32 [B+1] device tensor, graph b = rows [graph_ptr[b], graph_ptr[b+1]).
        want_den (training): -> (out, den float32 [N,H], sumsq float32 [2] = |Q|^2, |K|^2) for batched_simple_backward."""
        dev = _require_device(q, k, v, graph_ptr)
        N, H, M = q.shape
        D = v.shape[2]
        _all_f32(q=q, k=k, v=v)
        if graph_ptr.dtype != torch.int32 or not graph_ptr.is_contiguous():
            raise TypeError("difformer_amd: graph_ptr must be a contiguous int32 tensor [B+1]")
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        out = torch.empty((N, H, D), dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_batched_simple_workspace_bytes()
        ws = _workspace(ws_bytes, dev)
        head = (_ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(graph_ptr), graph_ptr.numel() - 1, N, H, M, D, _ptr(out),
                H * D)
        if want_den:                         # the _fwd_ symbol takes `den` between the output and the workspace
            den = torch.empty((N, H), dtype=torch.float32, device=dev)
            self._call("dif_batched_simple_attn_fwd_f32", "dif_batched_simple_attn_fwd_f32", dev, *head, _ptr(den),
                       _ptr(ws), ws_bytes)
            return out, den, ws.view(torch.float32)[-2:].clone()
        self._call("dif_batched_simple_attn_f32", "dif_batched_simple_attn_f32", dev, *head, _ptr(ws), ws_bytes)
        return out

    def batched_simple_backward(self, q, k, v, out, den, sumsq, g, graph_ptr):
        """(dq, dk, dv) of batched_simple_attention: three launches of the forward kernel's raw mode
        (dif_batched_simple_raw_f32: per-graph sum of outer products applied to the graph's own rows) plus row-wise
        tensor arithmetic; formulas in include/difformer_hip.h."""
        dev = _require_device(q, k, v, out, den, sumsq, g, graph_ptr)
        N, H, M = q.shape
        D = v.shape[2]
        _all_f32(q=q, k=k, v=v, out=out, den=den, grad=g)
        q, k, v, g = _contig(q, k, v, g)
        gn = (g / den.unsqueeze(-1)).contiguous()
        gd = (-(g * out).sum(dim=-1) / den).contiguous()
        B = graph_ptr.numel() - 1

        def raw(a, b, c, rs, vw, vs_is_s):
            Ma, Dc = a.shape[2], c.shape[2]
            dst = torch.empty((N, H, Dc), dtype=torch.float32, device=dev)
            self._call("dif_batched_simple_raw_f32", "dif_batched_simple_raw_f32", dev, _ptr(a), H * Ma, _ptr(b), H * Ma,
                       _ptr(c), H * Dc, _ptr(graph_ptr), B, N, H, Ma, Dc, _ptr(sumsq), _ptr(rs), _ptr(vw), int(vs_is_s),
                       _ptr(dst), H * Dc)
            return dst

        dq = raw(gn, v, k, gd, None, 1)                 # s gn (sum v (x) k) + s gd ksum_b
        T = (q * dq).sum()                              # s dL/ds (no cancellation: as in simple_backward)
        dk = raw(v, gn, q, None, gd, 1)                 # s v (sum gn (x) q) + s sum gd q
        dv = raw(k, q, gn, None, None, 0)               # s k (sum q (x) gn) + sum gn
        dq.addcmul_(q, (-T / sumsq[0]).expand_as(q))
        dk.addcmul_(k, (-T / sumsq[1]).expand_as(k))
        return dq, dk, dv

    def batched_sigmoid_attention(self, q, k, v, ranked_first, pos_count, want_den=False):
        """ranked_first: int32 [B] first row of the r-th largest graph; pos_count: int32 [max_nodes].
        want_den (training, D <= 64): -> (out, den float32 [N, H]) for batched_sigmoid_backward."""
        dev = _require_device(q, k, v, ranked_first, pos_count)
        N, H, M = q.shape
        D = v.shape[2]
        _all_f32(q=q, k=k, v=v)
        for t_ in (ranked_first, pos_count):
            if t_.dtype != torch.int32 or not t_.is_contiguous():
                raise TypeError("difformer_amd: ranked_first / pos_count must be contiguous int32 tensors")
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        out = torch.empty((N, H, D), dtype=torch.float32, device=dev)
        args = (_ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(ranked_first), _ptr(pos_count), ranked_first.numel(),
                pos_count.numel(), H, M, D, _ptr(out), H * D)
        if want_den:                         # the _fwd_ symbol takes `den` after the output
            den = torch.empty((N, H), dtype=torch.float32, device=dev)
            self._call("dif_batched_sigmoid_attn_fwd_f32", "dif_batched_sigmoid_attn_fwd_f32", dev, *args, _ptr(den))
            return out, den
        self._call("dif_batched_sigmoid_attn_f32", "dif_batched_sigmoid_attn_f32", dev, *args)
        return out

    def batched_sigmoid_backward(self, q, k, v, out, den, g, ranked_first, pos_count):
        """(dq, dk, dv) of the batched sigmoid attention (difformer-v2.py:113-135) for fp32 operands with M, D <= 64:
        csrc/sigmoid_attn_bwd.hip with the position groups' row mapping; nothing of size B x B x max_nodes is stored."""
        dev = _require_device(q, k, v, out, den, g, ranked_first, pos_count)
        N, H, M = q.shape
        D = v.shape[2]
        _all_f32(q=q, k=k, v=v, out=out, den=den, grad=g)
        q, ldq = _row_major(q, H * M)
        k, ldk = _row_major(k, H * M)
        v, ldv = _row_major(v, H * D)
        out, den, g = out.contiguous(), den.contiguous(), g.contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        dq, dk, dv = torch.empty((N, H, M), **f32), torch.empty((N, H, M), **f32), torch.empty((N, H, D), **f32)
        ws_bytes = self.lib.dif_batched_sigmoid_bwd_workspace_bytes(N, H)
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_batched_sigmoid_attn_bwd_f32", "dif_batched_sigmoid_attn_bwd_f32", dev, _ptr(q), ldq, _ptr(k), ldk,
                   _ptr(v), ldv, _ptr(out), H * D, _ptr(den), _ptr(g), H * D, _ptr(ranked_first), _ptr(pos_count),
                   ranked_first.numel(), pos_count.numel(), N, H, M, D, _ptr(dq), H * M, _ptr(dk), H * M, _ptr(dv), H * D,
                   _ptr(ws), ws_bytes)
        return dq, dk, dv

    # ---- a3 --------------------------------------------------------------------------------
    def csr_build(self, edge_index, edge_weight, num_nodes, n_blocks=1, transpose=False, block_rows=0):
        dev = _require_device(edge_index, edge_weight)
        _check_edge_index(edge_index)
        ei = edge_index.contiguous()
        E = int(ei.shape[1])
        ew = None
        if edge_weight is not None:
            ew = _f32(edge_weight, "edge_weight").contiguous()
            if ew.numel() != E:
                raise ValueError("difformer_amd: edge_weight must have one entry per edge")
        rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
        src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        val = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)          # {index out of range, longest row}
        blkptr = None
        if n_blocks > 1:
            blkptr = torch.empty((n_blocks + 1) * num_nodes, dtype=torch.int32, device=dev)
        ws_bytes = self.lib.dif_csr_workspace_bytes(E, num_nodes, n_blocks)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_csr_build", "dif_csr_build", dev, _ptr(ei), E, num_nodes, _ptr(ew), n_blocks, int(block_rows),
                   int(bool(transpose)), _ptr(rowptr), _ptr(blkptr), _ptr(src), _ptr(val), _ptr(status), _ptr(ws), ws_bytes)
        bad, longest = status.tolist()  # one sync per (cold) build; the longest row rides along (kernel selection)
        if bad != 0:
            raise IndexError(f"difformer_amd: edge_index holds node ids outside [0, {num_nodes})")
        return rowptr, blkptr, src, val, int(longest)

    def subgraph(self, subset, edge_index, edge_weight, num_nodes):
        """Induced subgraph with relabelling (main-batch.py:131) -> (edge_index [2,E'], edge_weight [E'] | None)."""
        dev = _require_device(subset, edge_index, edge_weight)
        if edge_index.dtype != torch.int64 or subset.dtype != torch.int64:
            raise TypeError("difformer_amd: subset and edge_index must be int64")
        ei = edge_index.contiguous()
        sub = subset.contiguous()
        E, B = int(ei.shape[1]), int(sub.numel())
        ew = None if edge_weight is None else _f32(edge_weight, "edge_weight").contiguous()
        if E == 0:                                             # nothing to filter (an empty tensor has no address to hand over)
            if B and bool(((sub < 0) | (sub >= num_nodes)).any()):
                raise IndexError(f"difformer_amd: subset / edge_index hold node ids outside [0, {num_nodes})")
            return (torch.empty((2, 0), dtype=torch.int64, device=dev),
                    None if ew is None else torch.empty(0, dtype=torch.float32, device=dev))
        out_ei = torch.empty((2, max(E, 1)), dtype=torch.int64, device=dev)
        out_w = None if ew is None else torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        res, count, status = _kept_status(dev)
        ws_bytes = self.lib.dif_subgraph_workspace_bytes(E, num_nodes)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_subgraph", "dif_subgraph", dev, _ptr(ei), E, num_nodes, _ptr(sub), B, _ptr(ew), _ptr(out_ei),
                   _ptr(out_w), _ptr(count), _ptr(status), _ptr(ws), ws_bytes)
        kept = _read_kept(res, "subset / edge_index hold", num_nodes)
        out = torch.stack([out_ei[0, :kept], out_ei[1, :kept]])
        return out, (None if out_w is None else out_w[:kept].clone())

    def graph_prepare(self, edge_index, num_nodes, undirected=False, remove_loops=False, add_loops=False):
        """to_undirected -> remove_self_loops -> add_self_loops (any subset, in that order) on the device -> [2, E']."""
        dev = _require_device(edge_index)
        _check_edge_index(edge_index)
        ei = edge_index.contiguous()
        E = int(ei.shape[1])
        cap = (2 * E if undirected else E) + (num_nodes if add_loops else 0)
        out = torch.empty((2, max(cap, 1)), dtype=torch.int64, device=dev)
        res, count, status = _kept_status(dev)
        ws_bytes = self.lib.dif_graph_prepare_workspace_bytes(E, num_nodes, int(bool(undirected)))
        ws = _workspace(ws_bytes, dev, floor=256)
        self._call("dif_graph_prepare", "dif_graph_prepare", dev, _ptr(ei), E, num_nodes, int(bool(undirected)),
                   int(bool(remove_loops)), int(bool(add_loops)), max(cap, 1), _ptr(out), _ptr(count), _ptr(status),
                   _ptr(ws), ws_bytes)
        kept = _read_kept(res, "edge_index holds", num_nodes)
        return torch.stack([out[0, :kept], out[1, :kept]])

    def subgraph_batches(self, perm, batch_size, edge_index, edge_weight, num_nodes, build_csr=False):
        """All induced subgraphs of an epoch (main-batch.py:121-131) from one pass over the edge list ->
        (edge_index [2, kept] grouped by batch, edge_weight [kept] | None, batch_ptr: python list of n_batches + 1 ints,
        csr | None) with csr = (rowptr int32 [M + 1], src int32 [kept], val float32 [kept]) over all batches when
        build_csr (one sort instead of one dif_csr_build per batch)."""
        dev = _require_device(perm, edge_index, edge_weight)
        if edge_index.dtype != torch.int64 or perm.dtype != torch.int64:
            raise TypeError("difformer_amd: perm and edge_index must be int64")
        ei, pm = edge_index.contiguous(), perm.contiguous()
        E, M = int(ei.shape[1]), int(pm.numel())
        nb = -(-M // int(batch_size))
        ew = None if edge_weight is None else _f32(edge_weight, "edge_weight").contiguous()
        bptr = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = self.lib.dif_subgraph_batches_workspace_bytes(E, num_nodes, nb)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_subgraph_batches", "dif_subgraph_batches_group", dev, _ptr(ei), E, num_nodes, _ptr(pm), M,
                   int(batch_size), _ptr(bptr), _ptr(status), _ptr(ws), ws_bytes)
        ptr = bptr.tolist()                                   # one sync per epoch: the result size is data dependent
        bad = int(status.item())
        if bad & 1:
            raise IndexError(f"difformer_amd: perm / edge_index hold node ids outside [0, {num_nodes})")
        if bad & 2:
            raise ValueError("difformer_amd: perm repeats a node id")
        kept = ptr[-1]
        out_ei = torch.empty((2, max(kept, 1)), dtype=torch.int64, device=dev)
        out_w = None if ew is None else torch.empty(max(kept, 1), dtype=torch.float32, device=dev)
        self._call("dif_subgraph_batches", "dif_subgraph_batches_emit", dev, _ptr(ei), E, num_nodes, M, int(batch_size),
                   _ptr(ew), _ptr(bptr), kept, _ptr(out_ei), _ptr(out_w), _ptr(ws), ws_bytes)
        csr = None
        if build_csr:
            rowptr = torch.empty(M + 1, dtype=torch.int32, device=dev)
            src = torch.empty(max(kept, 1), dtype=torch.int32, device=dev)
            val = torch.empty(max(kept, 1), dtype=torch.float32, device=dev)
            ws2_bytes = self.lib.dif_subgraph_batches_csr_workspace_bytes(kept, M)
            ws2 = _workspace(ws2_bytes, dev)
            self._call("dif_subgraph_batches", "dif_subgraph_batches_csr", dev, _ptr(ei), E, num_nodes, M, int(batch_size),
                       _ptr(ew), kept, _ptr(ws), ws_bytes, _ptr(rowptr), _ptr(src), _ptr(val), _ptr(ws2), ws2_bytes)
            csr = (rowptr, src, val)
        return out_ei[:, :kept], (None if out_w is None else out_w[:kept]), ptr, csr

    def edge_weight_grad(self, edge_index, edge_weight, rowptr, n_nodes, g, x, scale=1.0):
        """d loss / d edge_weight of the aggregation (difformer.py:73 under autograd): g, x [n_nodes, F] -> [E]."""
        dev = _require_device(edge_index, edge_weight, rowptr, g, x)
        _check_edge_index(edge_index)
        E, F = edge_index.shape[1], x.shape[1]
        if g.shape != x.shape or x.shape[0] != n_nodes:
            raise ValueError(f"difformer_amd: edge_weight_grad needs g and x as [{n_nodes}, F] (got {tuple(g.shape)}, {tuple(x.shape)})")
        _all_f32(g=g, x=x)
        w = _f32(edge_weight, "edge_weight").detach().contiguous()
        ei = edge_index.contiguous()
        g, ldg = _row_major(g, F)
        x, ldx = _row_major(x, F)
        dw = torch.empty(E, dtype=torch.float32, device=dev)
        self._call("dif_gcn_edge_weight_grad_f32", "dif_gcn_edge_weight_grad_f32", dev, _ptr(ei), E, n_nodes, _ptr(w),
                   _ptr(rowptr), _ptr(g), ldg, _ptr(x), ldx, F, float(scale), _ptr(dw))
        return dw

    def spmm(self, rowptr, blkptr, n_blocks, src, val, n_nodes, nnz, x, row_begin, n_rows, attn=None, attn_scale=1.0,
             gcn_scale=1.0, tail=None, order=None, part=None):
        """tail = None | dict(x0, prev, alpha, ln_weight, ln_bias, eps[, relu]): fuse the layer tail (H == 1).
        part = None | (0 | 1, own_blk_begin, own_blk_end, scratch | None, x_row0): one half of a split product
        (row-sharded runs).  Part 0 takes `x` = this rank's OWN value rows, whose first row is source row x_row0 (the
        sources of blocks own_blk_begin .. own_blk_end-1), parks the accumulators and returns the scratch tensor; part 1
        takes all n_nodes gathered rows plus that scratch and returns the finished rows.
        order = None | (int32 [n_rows], n_split) from row_order(): degree-sorted rows (the first n_split of them split
        over a whole quad) for the blocked kernel's load balance."""
        order, n_split = order if order is not None else (None, 0)
        dev = _require_device(rowptr, blkptr, src, val, x, attn, order)
        if order is not None and (order.dtype != torch.int32 or order.numel() != n_rows or not order.is_contiguous()):
            raise TypeError("difformer_amd: order must be a contiguous int32 tensor with one entry per local row")
        F = x.shape[1]
        t = tail or {}
        x0, prev, lw, lb = t.get("x0"), t.get("prev"), t.get("ln_weight"), t.get("ln_bias")
        _require_device(x0, prev, lw, lb)
        dt, sfx = _storage(x, attn, x0, prev, lw, lb)
        _f32(val, "CSR values")
        x, ldx = _row_major(x, F)
        phase, own_lo, own_hi, scratch, x_row0 = part if part is not None else (None, 0, 0, None, 0)
        if phase != 0 and x.shape[0] != n_nodes:
            raise ValueError(f"difformer_amd: spmm needs all {n_nodes} source rows, got {x.shape[0]}")
        attn, lda = _rows(attn, F)
        x0, ldx0 = _rows(x0, F)
        prev, ldp = _rows(prev, F)
        lw, lb = _contig(lw, lb)
        out = torch.empty((n_rows, F), dtype=dt, device=dev)
        head = (_ptr(rowptr), _ptr(blkptr), n_blocks, _ptr(src), _ptr(val), n_nodes, nnz, _ptr(x), ldx, row_begin, n_rows, F,
                _ptr(attn), lda, float(attn_scale), float(gcn_scale), _ptr(order), int(n_split))
        tail_args = (_ptr(x0), ldx0, _ptr(prev), ldp, float(t.get("alpha", 0.5)), _ptr(lw), _ptr(lb),
                     float(t.get("eps", 1e-5)), int(bool(t.get("relu", False))))
        if part is not None:
            sbytes = self.lib.dif_gcn_spmm_part_scratch_bytes(n_rows, int(n_split), F)
            if scratch is None:
                scratch = _workspace(sbytes, dev)
            # part 0 indexes x by GLOBAL source row but only ever touches this rank's own rows: hand it the pointer
            # the first own row would have inside a full [n_nodes, F] array
            xp = ctypes.c_void_p(x.data_ptr() - int(x_row0) * ldx * x.element_size())
            head = head[:7] + (xp,) + head[8:]
            self._call("dif_gcn_spmm_f32", "dif_gcn_spmm_part_" + sfx, dev, *head, int(tail is not None), *tail_args,
                       int(phase), int(own_lo), int(own_hi), PART0_WORKGROUPS if phase == 0 else 0, _ptr(scratch), sbytes,
                       _ptr(out), F)
            return scratch if phase == 0 else out
        if sfx == "bf16":
            symbol, args = "dif_gcn_spmm_tail_bf16", head + (int(tail is not None),) + tail_args
        elif tail is None:
            symbol, args = "dif_gcn_spmm_f32", head
        else:
            symbol, args = "dif_gcn_spmm_tail_f32", head + tail_args
        self._call("dif_gcn_spmm_f32", symbol, dev, *args, _ptr(out), F)
        return out

    # ---- a1 + a4 + tail in closed form (csrc/simple_layer.hip) ---------------------------------------------------------
    def gram(self, x, rowptr=None, plan=None):
        """x [n, C] fp32 -> (record [C*C + C + 2] = {X^T X, column sums}, ys | None).  With rowptr + plan the pass also
        writes the slice-major copy of x scaled by deg^-1/2 that sliced_spmm reads."""
        dev = _require_device(x, rowptr)
        dt, sfx = _storage(x)
        n, C = x.shape
        x, ldx = _rows(x, C, align=True)
        record = torch.empty(C * C + C + 2, dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_gram_workspace_bytes(n, C)
        ws = _workspace(ws_bytes, dev, floor=16)
        if sfx == "bf16":        # bfloat16 rows, float32 record; no slice-major copy (the sliced product is float32-only)
            if plan is not None:
                raise TypeError("difformer_amd: the slice-major copy of the sliced product is float32-only")
            self._call("dif_gram_f32", "dif_gram_bf16", dev, _ptr(x), ldx, n, C, _ptr(record), _ptr(ws), ws_bytes)
            return record, None
        ys = None if plan is None else _slice_major(C, plan, dev)
        self._call("dif_gram_f32", "dif_gram_f32", dev, _ptr(x), ldx, n, C, _ptr(rowptr) if plan is not None else None,
                   plan, _ptr(ys), _ptr(record), _ptr(ws), ws_bytes)
        return record, ys

    def input_gram(self, x, weight, bias, ln_weight, ln_bias, eps, relu, rowptr=None, plan=None, rows=True):
        """Input layer + the first closed-form layer's products in one pass (csrc/simple_layer.hip, input_gram_kernel):
        x [n, C_in <= 64] fp32 -> (h = ReLU(LayerNorm(x W^T + b)) [n, D], record of h as `gram` leaves it, ys | None).
        rows=False (single copy; needs plan): h is not stored, the hidden rows exist as ys alone -> (None, record, ys)."""
        dev = _require_device(x, weight, bias, ln_weight, ln_bias, rowptr)
        _all_f32(x=x, weight=weight, bias=bias)
        n, C = x.shape
        D = weight.shape[0]
        x, ldx = _row_major(x, C)
        weight, bias, ln_weight, ln_bias = _contig(weight, bias, ln_weight, ln_bias)
        if not rows and plan is None:
            raise TypeError("difformer_amd: input_gram(rows=False) leaves the rows as the slice-major copy: it needs rowptr and plan")
        out = torch.empty((n, D), dtype=torch.float32, device=dev) if rows else None
        record = torch.empty(D * D + D + 2, dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_gram_workspace_bytes(n, D)
        ws = _workspace(ws_bytes, dev, floor=16)
        ys = None if plan is None else _slice_major(D, plan, dev)
        self._call("dif_input_gram_f32", "dif_input_gram_f32", dev, _ptr(x), ldx, n, C, _ptr(weight), _ptr(bias), D,
                   _ptr(ln_weight), _ptr(ln_bias), float(eps), int(bool(relu)), _ptr(out), D,
                   _ptr(rowptr) if plan is not None else None, plan, _ptr(ys), _ptr(record), _ptr(ws), ws_bytes)
        return out, record, ys

    def simple_coeffs(self, record, n_global, C, D, Wq, bq, Wk, bk, Wv, bv, attn_scale):
        dev = _require_device(record, Wq, bq, Wk, bk, Wv, bv)
        ws_ = _contig(Wq, bq, Wk, bk, Wv, bv, f32="weight")
        coef = torch.empty(self.lib.dif_simple_coeffs_len(C, D), dtype=torch.float32, device=dev)
        self._call("dif_simple_coeffs_f32", "dif_simple_coeffs_f32", dev, _ptr(record), int(n_global), C, D,
                   *[_ptr(t) for t in ws_], float(attn_scale), _ptr(coef))
        return coef

    def gram_coeffs(self, x, n_global, C, D, Wq, bq, Wk, bk, Wv, bv, attn_scale):
        """gram(x) + simple_coeffs in one call (dif_gram_coeffs_f32): x [n, C] float32 -> (record, coef).  Up to 48 partial
        records of the Gram pass (<= 24,576 rows) are summed inside the coefficient kernel: two launches instead of three."""
        dev = _require_device(x, Wq, bq, Wk, bk, Wv, bv)
        _f32(x, "x")
        n = x.shape[0]
        x, ldx = _rows(x, C, align=True)
        ws_ = _contig(Wq, bq, Wk, bk, Wv, bv, f32="weight")
        record = torch.empty(C * C + C + 2, dtype=torch.float32, device=dev)
        coef = torch.empty(self.lib.dif_simple_coeffs_len(C, D), dtype=torch.float32, device=dev)
        ws_bytes = self.lib.dif_gram_workspace_bytes(n, C)
        ws = _workspace(ws_bytes, dev, floor=16)
        self._call("dif_gram_coeffs_f32", "dif_gram_coeffs_f32", dev, _ptr(x), ldx, n, C, D, *[_ptr(t) for t in ws_],
                   int(n_global), float(attn_scale), _ptr(coef), _ptr(record), _ptr(ws), ws_bytes)
        return record, coef

    def row_gemm(self, A, mat, bias=None, accumulate=None):
        """A [n, K] @ mat [K, C] (+ bias [C]) (+ accumulate [n, C]) in one pass over the rows (dif_rowgemm_f32; K <= 512,
        float32) -> [n, C], or None when the shape is not covered (the caller then uses the vendor GEMM)."""
        dev = _require_device(A, mat, bias, accumulate)
        n, K = A.shape
        C = mat.shape[1]
        if K > 512 or any(t_ is not None and t_.dtype != torch.float32 for t_ in (A, mat, bias, accumulate)):
            return None
        A, lda = _row_major(A, K)
        mat, bias = _contig(mat, bias)
        accumulate, ldc = _rows(accumulate, C)
        one = None
        if accumulate is not None:
            one = self._ones.get(dev)
            if one is None:
                one = self._ones[dev] = torch.ones(1, dtype=torch.float32, device=dev)
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        self._call("dif_rowgemm_f32", "dif_rowgemm_f32", dev, _ptr(A), lda, _ptr(mat), C, 0, 0, 1.0, _ptr(bias), None, None,
                   1.0, _ptr(accumulate), ldc, _ptr(one), n, 1, K, C, _ptr(out), C)
        return out

    def closed_form_attn_backward(self, x, coef, D, d, dx_in=None, row_sums=None):
        """Backward of att = (x Mn + cn) / (x u + cd) in one pass (csrc/simple_layer.hip, closed_form_attn_bwd_kernel):
        -> (d_num [n, D], d_den [n], dx [n, C] = dx_in + d_num Mn^T + d_den u^T, d_u [C] = x^T d_den, d_cd [] = sum d_den,
        rs_d [D] = row_sums^T d or None), or None when the shape is not covered."""
        dev = _require_device(x, coef, d, dx_in, row_sums)
        n, C = x.shape
        if C % 4 or D % 4 or C > 64 or D > 64 or any(t_ is not None and t_.dtype != torch.float32 for t_ in (x, coef, d, dx_in)):
            return None
        x, ldx = _row_major(x, C)
        d, ldd = _row_major(d, D)
        dx_in, ldi = _rows(dx_in, C)
        if any(ld % 4 for ld in (ldx, ldd, ldi)) or any(t_ is not None and t_.data_ptr() % 16 for t_ in (x, d, dx_in)):
            return None
        d_num = torch.empty((n, D), dtype=torch.float32, device=dev)
        d_den = torch.empty((n,), dtype=torch.float32, device=dev)
        dx = torch.empty((n, C), dtype=torch.float32, device=dev)
        if row_sums is not None:
            row_sums = _f32(row_sums, "row_sums").contiguous()
        parts = torch.empty((self.lib.dif_closed_form_attn_bwd_groups(n), 132), dtype=torch.float32, device=dev)
        self._call("dif_simple_layer_f32", "dif_closed_form_attn_bwd_f32", dev, _ptr(x), ldx, n, C, D, _ptr(coef), _ptr(d),
                   ldd, _ptr(dx_in), ldi, _ptr(d_num), _ptr(d_den), _ptr(dx), C, _ptr(row_sums), _ptr(parts))
        sums = parts.sum(dim=0)                      # one partial record per workgroup, added in a fixed order
        return d_num, d_den, dx, sums[:C], sums[128], (sums[64: 64 + D] if row_sums is not None else None)

    def simple_coeffs_backward(self, record, n_global, C, D, Wq, bq, Wk, bk, Wv, bv, attn_scale, coef, dcoef):
        """Backward of simple_coeffs in one launch (csrc/simple_coeffs_bwd.hip): dcoef in coef's layout ->
        (S [C, C], t [C], dWq, dbq, dWk, dbk, dWv | None, dbv | None): dx = x S + 1 t^T through the record."""
        dev = _require_device(record, Wq, bq, Wk, bk, Wv, bv, coef, dcoef)
        ws_ = _contig(Wq, bq, Wk, bk, Wv, bv, f32="weight")
        if dcoef.numel() < D * C + D + C + 1 or not dcoef.is_contiguous():
            raise TypeError("difformer_amd: dcoef must be contiguous with coef's layout [D*C | D | C | 1]")
        out = torch.empty(self.lib.dif_simple_coeffs_bwd_len(C, D), dtype=torch.float32, device=dev)
        self._call("dif_simple_coeffs_f32", "dif_simple_coeffs_bwd_f32", dev, _ptr(record), int(n_global), C, D,
                   *[_ptr(t_) for t_ in ws_], float(attn_scale), _ptr(_f32(coef, "coef")), _ptr(_f32(dcoef, "dcoef")),
                   _ptr(out))
        o = 0
        parts = []
        for shape in ((C, C), (C,), (D, C), (D,), (D, C), (D,), (D, C), (D,)):
            k = shape[0] * (shape[1] if len(shape) > 1 else 1)
            parts.append(out[o: o + k].view(shape))
            o += k
        if Wv is None:
            parts[6] = parts[7] = None
        return parts

    def simple_layer(self, x, coef, D, ax=None, Wv=None, bv=None, row_sums=None, gcn_scale=1.0, x0=None, residual=False,
                     alpha=0.5, ln_weight=None, ln_bias=None, eps=1e-5, relu=False, next_rowptr=None, next_plan=None,
                     head=None, gather=None, rscale=None, rows=True):
        """-> out [n, D]; with next_plan -> (out, ys): also the slice-major scaled copy of `out` for the next layer's SpMM
        (see gram()).
        head = (Wo [Co, D], bo [Co]) float32, Co <= 128 (the model's output Linear, difformer.py:208): -> logits [n, Co]
        from the same pass; the layer's rows themselves are not stored.
        gather = (rowptr, src, val) of a one-block CSR over the same n nodes: the aggregation runs inside the layer kernel
        (no `ax`, no `row_sums`, no next-layer products).
        rscale [n] float32 = deg^1/2 (single copy): x is not the rows [n, C] but their slice-major pre-scaled copy
        [C/4, rows per slice, 4] (`ys` of gram / input_gram / a previous layer).  rows=False (with next_plan): `out` is not
        stored either -> (None, ys)."""
        dev = _require_device(x, coef, ax, Wv, bv, row_sums, x0, ln_weight, ln_bias, rscale)
        if rscale is not None:
            if (gather is not None or x.dim() != 3 or x.shape[2] != 4 or x.dtype != torch.float32 or not x.is_contiguous() or
                    rscale.dtype != torch.float32 or not rscale.is_contiguous() or x.shape[1] < rscale.numel()):
                raise TypeError("difformer_amd: rscale goes with the contiguous float32 slice-major copy [C/4, rows, 4] of the "
                                "layer input and no in-kernel aggregation")
            n, C = rscale.numel(), 4 * x.shape[0]
        else:
            n, C = x.shape
        if not rows and (rscale is None or next_plan is None):
            raise TypeError("difformer_amd: simple_layer(rows=False) is the single-copy mode: it needs rscale and next_plan")
        if gather is not None:
            rowptr, src, val = gather
            if (ax is not None or next_plan is not None or rowptr.numel() != n + 1 or rowptr.dtype != torch.int32 or
                    src.dtype != torch.int32):
                raise TypeError("difformer_amd: the in-kernel aggregation takes an int32 one-block CSR over the rows of x "
                                "and neither ax nor next-layer products")
            _f32(val, "val")
            row_sums = None
        dt, sfx = _storage(x, ax, x0)              # activations: float32 or bfloat16; parameters always float32 here
        _all_f32(coef=coef, Wv=Wv, bv=bv, ln_weight=ln_weight, ln_bias=ln_bias, row_sums=row_sums)
        if rscale is not None:
            ldx = x.shape[1]                           # rows per slice
        else:
            x, ldx = _rows(x, C, align=True)
        ax, ldax = _rows(ax, C, align=True)
        x0, ldx0 = _rows(x0, D, align=True)
        Wv, bv, ln_weight, ln_bias = _contig(Wv, bv, ln_weight, ln_bias)
        Wo = bo = None
        Co = 0
        if head is not None:
            Wo, bo = _contig(*head, f32="head")                              # float32 (exact copies of bf16 parameters)
            Co = Wo.shape[0]
            if next_plan is not None or Co > 128 or Wo.shape[1] != D:
                raise TypeError("difformer_amd: the fused output Linear needs Co <= 128 and no next-layer products")
        # the argument runs that every symbol of the family shares: x ... coef in front, gcn_scale ... relu behind the
        # aggregation's operands
        front = (_ptr(x), ldx, n, C, D, _ptr(coef))
        tail = (float(gcn_scale), _ptr(x0), ldx0, int(bool(residual)), float(alpha), _ptr(ln_weight), _ptr(ln_bias),
                float(eps), int(bool(relu)))
        if gather is not None:
            csr = (_ptr(rowptr), _ptr(src), _ptr(val), _ptr(Wv), _ptr(bv))
            return self._simple_layer_gather(dev, dt, sfx, n, D, front + csr + tail, Wo, bo, Co)
        args = front + (_ptr(ax), ldax, _ptr(Wv), _ptr(bv), _ptr(row_sums)) + tail
        if head is not None:
            logits = torch.empty((n, Co), dtype=dt, device=dev)
            self._call("dif_simple_layer_f32", "dif_simple_layer_head_" + sfx, dev, *args, None, 0, _ptr(Wo), _ptr(bo), Co,
                       _ptr(logits), Co, *((_ptr(rscale),) if sfx == "f32" else ()))
            return logits
        out = torch.empty((n, D), dtype=dt, device=dev) if rows else None
        if sfx == "bf16":
            if next_plan is not None:
                raise TypeError("difformer_amd: products for the next layer are float32-only")
            self._call("dif_simple_layer_f32", "dif_simple_layer_bf16", dev, *args, _ptr(out), D)
            return out
        ys = None if next_plan is None else _slice_major(D, next_plan, dev)
        self._call("dif_simple_layer_f32", "dif_simple_layer_f32", dev, *args, _ptr(out), D,
                   _ptr(next_rowptr) if ys is not None else None, next_plan if ys is not None else None, _ptr(ys),
                   _ptr(rscale))
        return out if next_plan is None else (out, ys)

    def _simple_layer_gather(self, dev, dt, sfx, n, D, args, Wo, bo, Co):
        """The launch of simple_layer(gather=...): `args` up to `relu`, then the rows or, with a head, the logits."""
        out = logits = None
        if Wo is not None:
            logits = torch.empty((n, Co), dtype=dt, device=dev)
        else:
            out = torch.empty((n, D), dtype=dt, device=dev)
        self._call("dif_simple_layer_f32", "dif_simple_layer_gather_" + sfx, dev, *args, _ptr(out), D, _ptr(Wo), _ptr(bo),
                   Co, _ptr(logits), Co)
        return logits if Wo is not None else out

    # ---- a3, dense unweighted graphs: feature-sliced product with LDS-staged sources (csrc/gcn_sliced.hip) ----------
    def sliced_plan(self, n_src, n_rows, F):
        """The geometry (sliced.SlicedPlan, an int32[8] ctypes array) or None when the shape is not covered."""
        plan = SlicedPlan()
        rc = self.lib.dif_sliced_plan(int(n_src), int(n_rows), int(F), plan)
        return plan if rc == 0 else None

    def sliced_build(self, rowptr, blkptr, src, n_src, nnz, row_begin, n_rows, F, plan, order=None, parts=None, n_pos=None,
                     quad_cap=1, positions=False):
        """-> (entries uint16 [512 * n_blocks], table int32) or None when a (row position, tile) group exceeds the 16-bit
        counters.  order (int32), parts (uint16), n_pos, quad_cap, positions: as sliced.SlicedAdjacency holds them; plan =
        sliced_plan(n_src, n_pos, F).  quad_cap (1 = strict, conflict-free schedule; 2 = packed) and positions (one 8-byte
        record {row, deg^-1/2} per row position for the product's epilogue) go to the two build calls in flagged copies of
        the plan (sliced.SlicedPlan), the caller's plan stays as it is.  The records lie in FRONT of the blocks in one
        allocation; `entries` is the view behind them, so it has the same shape and content with and without records.
        Two host syncs (status, block count): cold path, once per (graph, shard, F)."""
        dev = _require_device(rowptr, blkptr, src, order, parts)
        n_pos = int(n_rows) if n_pos is None else int(n_pos)
        G, NT = plan.G, plan.NT
        plan = plan.with_capacity(quad_cap)
        emit_plan = plan.with_records(positions)             # only dif_sliced_emit (and the product) take the records bit
        i32 = dict(dtype=torch.int32, device=dev)
        srt = torch.empty(max(int(nnz), 1), dtype=torch.int16, device=dev)
        counts = torch.empty(n_pos * NT * 32, dtype=torch.uint8, device=dev)
        lengths = torch.empty(G * NT * 4, **i32)
        table = torch.empty((plan.R + 1) * plan.panels * NT * plan.W + 1, **i32)
        status = torch.empty(1, **i32)
        self._call("dif_sliced_measure", "dif_sliced_measure", dev, _ptr(rowptr), _ptr(blkptr), _ptr(src), int(n_src),
                   int(nnz), int(row_begin), int(n_rows), int(F), plan, _ptr(order), _ptr(parts), n_pos, _ptr(srt),
                   _ptr(counts), _ptr(lengths), _ptr(table), _ptr(status))
        bad, n_blocks = (int(v) for v in torch.stack([status[0], table[-1]]).tolist())
        if bad:
            return None
        head = emit_plan.record_elems
        entries = torch.empty(head + 512 * max(n_blocks, 1), dtype=torch.int16, device=dev)
        if head:
            entries = entries[head:]
        self._call("dif_sliced_emit", "dif_sliced_emit", dev, _ptr(rowptr), _ptr(blkptr), int(n_src), int(row_begin),
                   int(n_rows), int(F), emit_plan, _ptr(order), _ptr(parts), n_pos, _ptr(srt), _ptr(counts), _ptr(table),
                   max(n_blocks, 1), _ptr(entries))
        return entries, table

    def sliced_slot_order(self, rowptr, blkptr, n_src, row_begin, n_rows, plan):
        """Rows of the shard in the dealt order of the packed schedule (csrc/sliced_slots.hip, include/difformer_slots.h):
        int32 [n_rows] on the device, no host sync -- or None for a geometry the call does not cover (more than 18 tiles,
        or (panel, wave) pairs x tiles beyond the deal's LDS) or when libdifformer_slots.so is not there."""
        if not os.path.exists(_lib.SLOTS_LIB_PATH):
            return None
        dev = _require_device(rowptr, blkptr)
        ws_bytes = _lib.load_slots().dif_sliced_slot_order_workspace_bytes(int(n_rows), plan)
        if ws_bytes <= 0:
            return None
        order = torch.empty(int(n_rows), dtype=torch.int32, device=dev)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_sliced_slot_order", "dif_sliced_slot_order", dev, _ptr(rowptr), _ptr(blkptr), int(n_src), int(row_begin),
                   int(n_rows), plan, _ptr(order), _ptr(ws), ws_bytes, slots=True)
        return order

    def sliced_prescale(self, x, rowptr, n_src, plan, dinv=None):
        """x [n_src, F] fp32 -> ys [F/4, T*NT, 4]: rows scaled by deg^-1/2 (dinv, or from the row lengths), slice-major."""
        dev = _require_device(x, rowptr, dinv)
        _f32(x, "x")
        F = x.shape[1]
        x, ldx = _rows(x, F, align=True)
        ys = _slice_major(F, plan, dev)
        self._call("dif_sliced_prescale_f32", "dif_sliced_prescale_f32", dev, _ptr(x), ldx, _ptr(rowptr), _ptr(dinv),
                   int(n_src), F, plan, _ptr(ys))
        return ys

    def sliced_spmm(self, sl, ys, rowptr, n_src, row_begin, n_rows, F, attn=None, attn_scale=1.0, gcn_scale=1.0, dinv=None):
        """sl: the format (sliced.SlicedAdjacency: entries, table, run_plan, order, parts, n_pos) built for these rows."""
        dev = _require_device(sl.entries, sl.table, ys, rowptr, attn, sl.order, sl.parts, dinv)
        _all_f32(attn=attn)
        attn, lda = _rows(attn, F, align=True)
        out = torch.empty((n_rows, F), dtype=torch.float32, device=dev)
        n_pos = int(n_rows) if sl.n_pos is None else int(sl.n_pos)
        ws_bytes = self.lib.dif_sliced_spmm_workspace_bytes(int(n_src), n_pos, int(F))   # > 0: a row shard (source splits)
        ws = _workspace(ws_bytes, dev, or_none=True)
        if sl.entries.storage_offset() < sl.run_plan.record_elems:      # (0 for a format built without position records)
            raise ValueError("difformer_amd: this sliced format has lost the position records in front of its entries")
        self._call("dif_sliced_spmm_f32", "dif_sliced_spmm_f32", dev, _ptr(sl.entries), _ptr(sl.table), sl.run_plan, _ptr(ys),
                   _ptr(rowptr), _ptr(dinv), _ptr(sl.order), _ptr(sl.parts), n_pos, int(n_src), int(row_begin), int(n_rows),
                   int(F), _ptr(attn), lda, float(attn_scale), float(gcn_scale), _ptr(out), F, _ptr(ws), ws_bytes)
        return out

    def row_order(self, rowptr, row_begin, n_rows):
        """Rows [row_begin, row_begin + n_rows) by descending degree (indices inside the shard) ->
        (order int32 [n_rows], stats int32 [2] = {rows with degree > 4x mean, max degree}), both on the device."""
        dev = _require_device(rowptr)
        order = torch.empty(n_rows, dtype=torch.int32, device=dev)
        stats = torch.empty(2, dtype=torch.int32, device=dev)
        ws_bytes = self.lib.dif_row_order_workspace_bytes(n_rows)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_row_order", "dif_row_order", dev, _ptr(rowptr), row_begin, n_rows, _ptr(order), _ptr(stats),
                   _ptr(ws), ws_bytes)
        return order, stats

    # ---- a5 ends: narrow Linear (+ LayerNorm + ReLU) -------------------------------------------
    def linear(self, x, weight, bias, ln_weight=None, ln_bias=None, eps=1e-5, relu=False):
        dev = _require_device(x, weight, bias, ln_weight, ln_bias)
        n, C = x.shape
        Co = weight.shape[0]
        dt, sfx = _storage(x, weight, bias, ln_weight, ln_bias)
        x, ldx = _rows(x, C, align=C > 128)                                      # long rows: 4-element aligned rows
        weight, bias, ln_weight, ln_bias = _contig(weight, bias, ln_weight, ln_bias)
        out = torch.empty((n, Co), dtype=dt, device=dev)
        from . import ops
        if sfx == "f32" and Co > 64 and ops.linear_xwide_covers(x, weight):
            # wide rows into a wide layer: one product (C <= 416) or the two halves of the input channels as the two accumulating
            # products of the hidden-300 layer kernel; weights packed once per parameter version
            x, ldx = _rows(x, C, align=True)
            two = C > ops.XWIDE_MAX
            Ch = C // 2 if two else C
            pa = self.xwide_pack(weight, False, Ch, Co, cache=True)
            pb = self.xwide_pack(weight, False, Ch, Co, cache=True, col0=Ch) if two else None
            symbol, mats = "dif_linear_xwide_f32", (_ptr(pa), _ptr(pb))
        elif (sfx == "f32" and C > 128 and Co <= 64 and C <= 8192 and not ops.EXACT_FP32 and
                (n < 16384 or C % 4 or ldx % 4 or x.data_ptr() % 16 or weight.data_ptr() % 16)):
            # few rows, or rows that are only 4-byte aligned (Cora: 2,708 x 1,433): K split over the waves of a workgroup,
            # the weights packed once per parameter version (bfloat16 hi / lo parts in MFMA fragment order)
            packed = self._packed_weight(weight, C, Co, dev)
            symbol, mats = "dif_linear_packed_f32", (_ptr(packed),)
        else:
            symbol, mats = "dif_linear_" + sfx, (_ptr(weight),)
        self._call("dif_linear_f32", symbol, dev, _ptr(x), ldx, n, C, *mats, _ptr(bias), Co, _ptr(ln_weight), _ptr(ln_bias),
                   float(eps), int(bool(relu)), _ptr(out), Co)
        return out

    def _cached_pack(self, tensor, geometry, pack):
        """pack() -> packed copy of a weight `tensor`, cached per tensor and `geometry` (a tuple) in a TensorCache (a new
        tensor at a recycled address must not find the old packing).  Rebuilt after optimiser steps / load_state_dict (they
        bump the version, and the insert drops the older version's entry: an optimiser step per epoch adds none); `.data`
        writes need model.invalidate_caches(); a tensor without a version is packed every time.  The cache is never emptied
        behind a captured hipGraph's back: a capture bakes raw pointers to these buffers in and pins the ones it used
        itself (`capture_pins`)."""
        packed = self._packed.lookup((tensor,), geometry)
        if packed is MISS:
            packed = self._packed.insert((tensor,), geometry, pack())
        return self._pin(packed)

    def _packed_weight(self, weight, C, Co, dev):
        """dif_linear_pack_f32 of a [Co, C] float32 weight, once per parameter version (_cached_pack)."""
        def pack():
            packed = torch.empty(self.lib.dif_linear_packed_bytes(C), dtype=torch.uint8, device=dev)
            self._call("dif_linear_pack_f32", "dif_linear_pack_f32", dev, _ptr(weight), C, Co, _ptr(packed))
            return packed
        return self._cached_pack(weight, (C, Co, str(dev)), pack)

    def _pin(self, packed):
        """While a forward is being captured, the capture keeps every packed buffer it was handed alive (DIFFormer.
        _forward_graphed / graphs.GraphedForward set `capture_pins` to a list around the capture)."""
        pins = getattr(self, "capture_pins", None)
        if pins is not None:
            pins.append(packed)
        return packed

    # ---- a4 / a5 tail ----------------------------------------------------------------------
    def layer_tail_bwd(self, conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu, grad_out, want):
        """Backward of layer_tail in one pass (csrc/layer_tail_bwd.hip).  want = (conv, x0, prev) booleans.
        -> (d_conv [n,H,D] | None, d_x0 | None, d_prev | None, d_ln_weight | None, d_ln_bias | None); None when the
        shape is not covered (D % 4 != 0, D > 512, bf16 storage): the caller re-derives the gradient with tensor ops."""
        dev = _require_device(conv, x0, prev, ln_weight, ln_bias, grad_out)
        n, H, D = conv.shape
        if D % 4 or D > 512 or any(t is not None and t.dtype != torch.float32 for t in (conv, x0, prev, ln_weight, grad_out)):
            return None
        conv, ldc = _row_major(conv, H * D)
        g, ldg = _row_major(grad_out, D)
        x0, ldx0 = _rows(x0, D)
        prev, ldp = _rows(prev, D)
        if any(ld % 4 for ld in (ldc, ldg, ldx0, ldp)) or any(t is not None and t.data_ptr() % 16 for t in (conv, g, x0, prev)):
            return None
        f32 = dict(dtype=torch.float32, device=dev)
        d_conv = torch.empty((n, H, D), **f32) if want[0] else None
        d_x0 = torch.empty((n, D), **f32) if (want[1] and x0 is not None) else None
        d_prev = torch.empty((n, D), **f32) if (want[2] and prev is not None) else None
        d_ln = ws = None
        ws_bytes = 0
        if ln_weight is not None:
            ln_weight, ln_bias = ln_weight.contiguous(), ln_bias.contiguous()
            d_ln = torch.empty(2 * D, **f32)
            ws_bytes = self.lib.dif_layer_tail_bwd_workspace_bytes(n, D)
            ws = _workspace(ws_bytes, dev)
        self._call("dif_layer_tail_bwd_f32", "dif_layer_tail_bwd_f32", dev, _ptr(conv), ldc, n, H, D, _ptr(x0), ldx0,
                   _ptr(prev), ldp, float(alpha), _ptr(ln_weight), _ptr(ln_bias), float(eps), int(bool(relu)), _ptr(g), ldg,
                   _ptr(d_conv), H * D, _ptr(d_x0), D, _ptr(d_prev), D, _ptr(d_ln), _ptr(ws), ws_bytes)
        return (d_conv, d_x0, d_prev, None if d_ln is None else d_ln[:D], None if d_ln is None else d_ln[D:2 * D])

    def coeffs_bg(self, x, record, n_global, factors, C, D, attn_scale, rscale=None):
        """Coefficients of the closed-form layer through the background kernels (csrc/side_chain.hip), enqueued on the
        CURRENT stream (the caller puts a side stream there): from x [n, C] (one pass: Gram partials per wave), or from a
        finished `record` [X^T X | sum x] when the layer input's Gram pass has already run.  factors:
        ops.NarrowFactors (pt, vtt, st float32 [80 * 80]).  -> coef (layout of simple_coeffs).
        rscale [n] (single copy): x is the slice-major pre-scaled copy [C/4, rows per slice, 4] of the rows, as for simple_layer."""
        dev = _require_device(x, record, factors.pt, rscale)
        f32 = dict(dtype=torch.float32, device=dev)
        gt = torch.empty(80 * 80 + 400, **f32)           # G~ + 100 float64 pairs of partial norm products
        if record is not None:
            ws, ws_bytes, xp, ldx, n = record, record.numel() * 4, None, 0, 1
        else:
            _f32(x, "x")
            if rscale is not None:
                if x.dim() != 3 or x.shape != (C // 4, x.shape[1], 4) or not x.is_contiguous() or x.shape[1] < rscale.numel():
                    raise TypeError("difformer_amd: rscale goes with the contiguous slice-major copy [C/4, rows, 4]")
                n, ldx = rscale.numel(), x.shape[1]
                rscale = _f32(rscale, "rscale").contiguous()
            else:
                n = x.shape[0]
                x, ldx = _rows(x, C, align=True)
            ws_bytes = self.lib.dif_gram_bg_workspace_bytes(n, C)
            ws = _workspace(ws_bytes, dev, floor=16)
            xp = x
        self._call("dif_gram_bg_f32", "dif_gram_bg_f32", dev, _ptr(xp), ldx, n, C, int(n_global), _ptr(factors.st), _ptr(gt),
                   _ptr(ws), ws_bytes, _ptr(rscale) if xp is not None else None)
        scratch = torch.empty(80 * 80 + 4, **f32)
        coef = torch.empty(self.lib.dif_simple_coeffs_len(C, D), **f32)
        self._call("dif_simple_coeffs_bg_f32", "dif_simple_coeffs_bg_f32", dev, _ptr(gt), _ptr(factors.pt), _ptr(factors.vtt),
                   _ptr(factors.st), C, D, float(attn_scale), _ptr(scratch), _ptr(coef))
        return coef

    def gram_sym(self, x):
        """x [n, C] fp32 -> record [C*C + 2*C + 2]: X^T X (blocks of 64 on and above the diagonal valid) | sum x | unused
        (csrc/simple_attn.hip, dif_gram_sym_f32) -- the Gram record of the closed form at the scripts' widths."""
        dev = _require_device(x)
        _f32(x, "x")
        n, C = x.shape
        x, ldx = _row_major(x, C)
        rec = torch.empty(self.lib.dif_simple_reduced_len(1, C, C), dtype=torch.float32, device=dev)
        from . import ops
        if 64 < C <= 128 and C % 4 == 0 and ldx % 4 == 0 and x.data_ptr() % 16 == 0 and (ops.EXACT_FP32 or n < 4096):
            # hidden 128: one pass over x with the whole upper half of X^T X in a wave's registers (csrc/simple_layer_wide.hip)
            ws_fn, symbol = self.lib.dif_gram128_workspace_bytes, "dif_gram128_f32"
        else:
            ws_fn, symbol = self.lib.dif_gram_sym_workspace_bytes, "dif_gram_sym_f32"
        ws_bytes = ws_fn(n, C)
        ws = _workspace(ws_bytes, dev)
        self._call("dif_gram_sym_f32", symbol, dev, _ptr(x), ldx, n, C, _ptr(rec), _ptr(ws), ws_bytes)
        return rec

    def wide_coeffs(self, rec, C, n_global, S, V, P):
        """Record of gram_sym -> (B float32 [C, DV], bias float32 [DV]), the row GEMM's operands [Mn | u], [cn | cd]: both
        float64 products and their bookkeeping in two launches (dif_wide_coeffs_f64; no library GEMM)."""
        dev = _require_device(rec, S, V, P)
        DV = V.shape[1]
        T = torch.empty((C + 1, DV), dtype=torch.float64, device=dev)
        partial = torch.empty(2 * ((C + 16) // 16), dtype=torch.float64, device=dev)
        B = torch.empty((C, DV), dtype=torch.float32, device=dev)
        bias = torch.empty(DV, dtype=torch.float32, device=dev)
        self._call("dif_wide_coeffs_f64", "dif_wide_coeffs_f64", dev, _ptr(rec), C, int(n_global), _ptr(S), _ptr(V), _ptr(P),
                   DV, _ptr(T), _ptr(partial), _ptr(B), _ptr(bias))
        return B, bias

    def layer_tail_mix(self, Z, D, den_col, conv_scale, add, add_scale, rs, bv, x0, prev, alpha, ln_weight, ln_bias, eps,
                       relu=False):
        """Tail of the closed form at the scripts' widths (dif_layer_tail_mix_f32): Z [n, >= D + 1] fp32 holds the
        numerator in columns [0, D) and the denominator in column den_col; add [n, D] / rs [n] / bv [D] optional."""
        dev = _require_device(Z, add, rs, bv, x0, prev, ln_weight, ln_bias)
        n, ldz = Z.shape
        _all_f32(Z=Z, add=add, rs=rs, bv=bv, x0=x0, prev=prev)
        if not Z.is_contiguous() or ldz % 4:
            raise ValueError("difformer_amd: layer_tail_mix needs a contiguous Z with a row length that is a multiple of 4")
        add, lda = _rows(add, D, align=True)
        x0, ldx0 = _rows(x0, D, align=True)
        prev, ldp = _rows(prev, D, align=True)
        ln_weight, ln_bias, rs, bv = _contig(ln_weight, ln_bias, rs, bv)
        out = torch.empty((n, D), dtype=torch.float32, device=dev)
        den_ptr = None if den_col is None else Z.data_ptr() + 4 * int(den_col)
        self._call("dif_layer_tail_mix_f32", "dif_layer_tail_mix_f32", dev, _ptr(Z), ldz, den_ptr, ldz, float(conv_scale),
                   _ptr(add), lda, float(add_scale), _ptr(rs), _ptr(bv), n, D, _ptr(x0), ldx0, _ptr(prev), ldp, float(alpha),
                   _ptr(ln_weight), _ptr(ln_bias), float(eps), int(bool(relu)), _ptr(out), D)
        return out

    def simple_layer_wide(self, x, B, bias, D, attn_scale, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight, ln_bias,
                          eps, relu=False):
        """Closed-form `simple` layer for 64 < max(C, D) <= 128 in one pass (csrc/simple_layer_wide.hip): x [n, C], B [C, dv]
        = [Mn | u | ...], bias [dv] = [cn | cd | ...] (wide_coeffs), ax = A_hat x [n, C] or None, Wv [D, C] / bv [D] / rs [n]."""
        return self._simple_layer_wide(False, x, B, bias, D, attn_scale, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha,
                                       ln_weight, ln_bias, eps, relu)

    def simple_layer_xwide(self, x, B, bias, D, attn_scale, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight, ln_bias,
                           eps, relu=False):
        """Closed-form `simple` layer for 128 < max(C, D) <= 416 in one pass (csrc/simple_layer_xwide.hip); arguments as
        simple_layer_wide.  Mn is packed per call (it changes with the Gram record), Wv once per parameter version."""
        return self._simple_layer_wide(True, x, B, bias, D, attn_scale, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha,
                                       ln_weight, ln_bias, eps, relu)

    def _simple_layer_wide(self, xwide, x, B, bias, D, attn_scale, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight,
                           ln_bias, eps, relu):
        """Both wide layer kernels: the same operands, but the xwide one takes Mn and Wv as packed MFMA fragments."""
        dev = _require_device(x, B, bias, ax, Wv, bv, rs, x0, ln_weight, ln_bias)
        n, C = x.shape
        _all_f32(x=x, B=B, bias=bias, ax=ax, Wv=Wv, x0=x0)
        x, ldx = _rows(x, C, align=True)
        ax, ldax = _rows(ax, C, align=True)
        x0, ldx0 = _rows(x0, D, align=True)
        B, bias, bv, rs, ln_weight, ln_bias = _contig(B, bias, bv, rs, ln_weight, ln_bias)
        coeffs = (_ptr(B), int(B.shape[1]), _ptr(bias), float(attn_scale), _ptr(ax), ldax)
        if xwide:
            pm = self.xwide_pack(B, True, C, D)
            pv = None if Wv is None else self.xwide_pack(Wv, False, C, D, cache=True)
            symbol, mats = "dif_simple_layer_xwide_f32", (_ptr(pm), _ptr(pv)) + coeffs
        else:
            Wv, = _contig(Wv)
            symbol, mats = "dif_simple_layer_wide_f32", coeffs + (_ptr(Wv),)
        out = torch.empty((n, D), dtype=torch.float32, device=dev)
        self._call("dif_simple_layer_f32", symbol, dev, _ptr(x), ldx, n, C, D, *mats, _ptr(bv), _ptr(rs), float(gcn_scale),
                   _ptr(x0), ldx0, int(bool(residual)), float(alpha), _ptr(ln_weight), _ptr(ln_bias), float(eps),
                   int(bool(relu)), _ptr(out), D)
        return out

    def xwide_pack(self, src, transposed, C, D, cache=False, col0=0):
        """dif_xwide_pack_f32: src [C, ld] (transposed: the [Mn | u] operand) or [D, ld] (an nn.Linear weight; col0: the C
        input channels start at that column) -> packed MFMA fragments.  cache=True keeps the packing per weight tensor
        (identity + version, as _packed_weight)."""
        dev = src.device

        def pack():
            src_c = src.contiguous()
            packed = torch.empty(self.lib.dif_xwide_packed_bytes(C, D), dtype=torch.uint8, device=dev)
            self._call("dif_xwide_pack_f32", "dif_xwide_pack_f32", dev, src_c.data_ptr() + 4 * col0, int(src_c.shape[1]),
                       int(bool(transposed)), C, D, _ptr(packed))
            return packed
        if cache:
            return self._cached_pack(src, (C, D, bool(transposed), str(dev), col0), pack)
        return self._pin(pack())

    def layer_tail(self, conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu=False):
        dev = _require_device(conv, x0, prev, ln_weight, ln_bias)
        n, H, D = conv.shape
        dt, sfx = _storage(conv, x0, prev, ln_weight, ln_bias)
        conv, ldc = _row_major(conv, H * D)
        x0, ldx0 = _rows(x0, D)
        prev, ldp = _rows(prev, D)
        ln_weight, ln_bias = _contig(ln_weight, ln_bias)
        out = torch.empty((n, D), dtype=dt, device=dev)
        self._call("dif_layer_tail_f32", "dif_layer_tail_" + sfx, dev, _ptr(conv), ldc, n, H, D, _ptr(x0), ldx0, _ptr(prev),
                   ldp, float(alpha), _ptr(ln_weight), _ptr(ln_bias), float(eps), int(bool(relu)), _ptr(out), D)
        return out
