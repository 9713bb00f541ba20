"""Device-side `gen_trace` for graphs of the primitives whose `process_trace` runs on the GPU
(Add, Mul, Recip, Sqrt, Rem, LessThan with its range-check table, SumReduce, MaxReduce, Contiguous, the LUT ops
Sin / Exp2 / Log2 with their lookup tables, and the graph inputs,
with expanded ("fake") dimensions as in luminal's ShapeTracker): a small host mirror of
`LuminairGraph::gen_trace` (`crates/graph/src/graph.rs:161-604`) over `lmn_trace_elementwise` /
`lmn_trace_sum_reduce`.  Nodes execute in creation (= topological) order, every tensor stays in HBM
as int32 `Fixed<12>` values, each node appends its rows to its kind's device-resident table, and the
resulting pie feeds `lmn_prove` with `LMN_TABLE_ROWS_ON_DEVICE`.

Multiplicities follow HEAD (`crates/graph/src/op/prim.rs:66-83,1005-1006`): an op consumes each input
with multiplicity -1 and yields its output `num_consumers` times (0 for a final output); a graph input
is yielded `num_consumers` times by its Inputs rows — so the logup sums of a complete graph cancel.
`num_consumers` is expansion-adjusted as in `graph.rs:215-243`: a consumer that reads the tensor through a
view with expanded dimensions counts once per repetition of each element.
Float tensors enter through `input_float` and leave through `read_float`: the f32 -> fixed conversion of `CopyToStwo` and
its inverse run on the device (`lmn_trace_inputs_float`, `lmn_tensor_to_float`).
The graph front-end itself (luminal's compiler passes, shape tracking) is outside the hot-path scope; this is the
execution + table-fill step only."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import backend
from .pie import TraceTableKind

_NCOLS = {0: 15, 1: 16, 2: 13, 3: 12, 5: 14, 6: 15, 7: 13, 8: 16, 9: 12, 11: 12, 13: 22, 15: 7, 16: 11}
_LUT_OF = {3: ("sin", 4), 9: ("exp2", 10), 11: ("log2", 12)}     # op kind -> (LUT name, lookup-table kind)


class _SlabLease(backend.DeviceBuffer):
    """The one device allocation of a gen_trace call.  `free()` hands it back to the context's one-slot cache instead
    of hipFree, so that a stream of small graphs on one context does not pay a hipMalloc / hipFree pair (~0.1 ms) per
    graph; a lease that is still in use is never handed out again (the cache only holds returned slabs)."""

    def free(self):
        if self.ptr and self.owned:
            cached = getattr(self.ctx, "_graph_slab", None)
            if cached is None or cached.nbytes < self.nbytes:
                if cached is not None:
                    cached.free()
                self.ctx._graph_slab = backend.DeviceBuffer(self.ctx, self.ptr, self.nbytes)
            else:
                backend.DeviceBuffer.free(self)
        self.ptr = 0


class _SinkLease:
    """A `gen_trace(columns=True)` sink among the call's buffers: `free()` closes it, like any other allocation of the call."""

    def __init__(self, sink: "backend.RowSink"):
        self.sink = sink

    def free(self):
        self.sink.close()


def _lease_slab(ctx, need: int) -> _SlabLease:
    cached = getattr(ctx, "_graph_slab", None)
    if cached is not None and cached.nbytes >= need:
        ctx._graph_slab = None
        return _SlabLease(ctx, cached.ptr, cached.nbytes)
    b = ctx.alloc(need)
    return _SlabLease(ctx, b.ptr, b.nbytes)


_al = lambda nbytes: (nbytes + 255) & ~255


class _Stager:
    """The one slab of a walk over the graph (hipMalloc per node would dominate small graphs) and the host data that has to
    reach it - graph inputs, LUT output columns, zeroed multiplicity tables and counters: packed into ONE staging array, each
    part 256-byte aligned, and uploaded with one copy (one synchronisation instead of one per tensor).  The staged bytes are
    the slab's first carve; tables and tensors are carved behind them."""

    def __init__(self):
        self.parts, self.off, self.nbytes, self.staged = [], {}, 0, None

    def stage(self, key, arr):
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint32)
        self.off[key] = (self.nbytes, a.nbytes)
        self.parts.append(a)
        if _al(a.nbytes) > a.nbytes:
            self.parts.append(np.zeros((_al(a.nbytes) - a.nbytes) // 4, dtype=np.uint32))
        self.nbytes += _al(a.nbytes)

    def stage_input(self, n: "_Node", host, fsrc):
        """a graph input's values: int32 `host`, or the raw bits of a float source that does not lie on the device yet"""
        if n.host is not None:
            self.stage(("in", n.out.node_id), host.astype(np.int32, copy=False))
        elif fsrc is not None and fsrc.tensor is None:
            self.stage(("in", n.out.node_id), _words(fsrc.host))

    def lease(self, ctx, carved_bytes: int) -> _SlabLease:
        self.slab, self.cursor = _lease_slab(ctx, carved_bytes + self.nbytes), 0
        return self.slab

    def upload(self, ctx):
        if self.nbytes:
            self.staged = ctx.upload_to(self.carve(self.nbytes), np.concatenate(self.parts))

    def dev_of(self, key) -> backend.DeviceBuffer:
        return self.staged.view(*self.off[key])

    def carve(self, nbytes: int) -> backend.DeviceBuffer:
        v = self.slab.view(self.cursor, nbytes)
        self.cursor += _al(nbytes)
        return v


def _refused_error(n_refused: int) -> ValueError:
    return ValueError("dry run: %d elements refused (a value outside [-(2^30-1), 2^30-1], Recip of a value <= 0, Sqrt of a "
                      "negative value, Rem outside lhs >= 0 and rhs > 0, or a LUT input outside its range)" % n_refused)


@dataclass(eq=False)          # a tensor is itself (a key of gen_trace_many's `feeds`), not its fields
class GraphTensor:
    node_id: int
    shape: Tuple[int, ...]
    consumers: int = 0
    is_output: bool = False
    buf: Optional[backend.DeviceBuffer] = None     # set by gen_trace / gen_trace_many
    member_stride: int = 0                         # gen_trace_many: elements between members in `buf` (0: one shared tensor)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))


@dataclass
class TensorView:
    """A tensor seen through a shape with expanded dimensions (stride 0), slices (offset) or permuted strides: the
    part of luminal's ShapeTracker the ops' index expressions need."""
    base: GraphTensor
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]
    offset: int = 0

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    @property
    def expansion(self) -> int:
        return int(np.prod([d for d, st in zip(self.shape, self.strides) if st == 0 and d > 1] or [1]))


def _as_view(t) -> TensorView:
    if isinstance(t, TensorView):
        return t
    strides, acc = [], 1
    for d in reversed(t.shape):
        strides.append(acc)
        acc *= d
    return TensorView(t, t.shape, tuple(reversed(strides)))


def _lmn_view(v: TensorView):
    """the `lmn_view` of a TensorView; None for the whole tensor in its own order"""
    if v.strides == _as_view(v.base).strides and v.shape == v.base.shape and not v.offset:
        return None
    return backend.LmnView.make(v.shape, v.strides, v.offset)


def _padded_lut_range(name: str, buf_min: int, buf_max: int) -> Tuple[int, int]:
    """`compute_padded_range_from_srcs` (crates/graph/src/utils.rs:44-82) for one Sin / Exp2 / Log2 node: the min..max of
    its source buffer padded by 10 % of the span, rounded to nearest; log2 clipped at the smallest positive value."""
    S = 4096.0
    lo_f, hi_f = float(buf_min) / S, float(buf_max) / S
    delta = (hi_f - lo_f) * 0.10
    rnd = lambda x: int(np.floor(abs(x) * S + 0.5)) * (1 if x >= 0 else -1)
    lo, hi = rnd(lo_f - delta), rnd(hi_f + delta)
    if name == "log2":
        lo = max(lo, 1)
    return lo, hi


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _words(arr: np.ndarray) -> np.ndarray:
    """an array's bytes as uint32 words, zero-padded to a whole word (2-byte elements of odd count)"""
    b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    if b.nbytes % 4:
        b = np.concatenate([b, np.zeros(4 - b.nbytes % 4, dtype=np.uint8)])
    return b.view(np.uint32)


class _FloatSource:
    """The float tensor behind an `input_float` node or a float feed: raw float bits, either on the host (`host`: float32 /
    float16, or uint16 bf16 patterns) or in a torch tensor on the context's device (`tensor`, kept alive here and read
    where it lies)."""

    def __init__(self, ctx, values, what: str):
        self.host, self.tensor = None, None
        if _is_torch(values):
            import torch
            self.code = backend.float_dtype_code(values.dtype)
            t = values.detach().contiguous()
            self.shape = tuple(int(d) for d in t.shape)
            if t.is_cuda:
                if t.device.index != ctx.device:
                    raise ValueError("%s: the tensor lives on %s, the context on device %d" % (what, t.device, ctx.device))
                self.tensor = t
            else:
                self.host = t.view(torch.int16).numpy().view(np.uint16) if self.code == backend.BF16 else t.numpy()
        else:
            v = np.asarray(values)
            self.code = backend.float_dtype_code(v.dtype)
            self.host = np.ascontiguousarray(v)
            self.shape = tuple(int(d) for d in v.shape)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    def on_host(self) -> np.ndarray:
        """the raw bits on the host (a device tensor comes down: one copy per call)"""
        if self.tensor is None:
            return self.host
        import torch
        t = self.tensor.cpu()
        return t.view(torch.int16).numpy().view(np.uint16) if self.code == backend.BF16 else t.numpy()

    def fixed(self) -> np.ndarray:
        """the Fixed<12> integers (`backend.to_fixed`: ValueError for what the device refuses)"""
        return backend.to_fixed(self.on_host(), backend.BF16 if self.code == backend.BF16 else None)


@dataclass
class _Node:
    kind: int
    out: GraphTensor
    inputs: List[GraphTensor]
    host: Optional[np.ndarray] = None      # graph inputs
    axis: int = 0                          # SumReduce
    per_member: bool = False               # graph inputs: one tensor per member of gen_trace_many (fed through `feeds`)
    fsrc: Optional[_FloatSource] = None    # graph inputs made by input_float (`host` is None then)


_REDUCES = (int(TraceTableKind.SumReduce), int(TraceTableKind.MaxReduce))
_LESS_THAN = int(TraceTableKind.LessThan)


def _ref_contig(n: "_Node") -> bool:
    """a Contiguous node in the reference's buffer rule (no expanded dimension)"""
    return n.kind == int(TraceTableKind.Contiguous) and n.inputs[0].expansion == 1


def _rows_of(n: "_Node") -> int:
    if n.kind in _REDUCES:
        return n.inputs[0].size
    if _ref_contig(n):
        return max(n.inputs[0].base.size, n.out.size)
    return n.out.size


class _Call:
    """What one node's producer call computes, whatever its destination: the producer (`op`), the operand buffers with
    their base tensors and views, and what only that producer reads - the reduce's (front, dim, back), the LUT's name,
    the float source's dtype.  `staged`: the staged values of a graph input; `fsrc`: the float source to read, if any.
    The emitters below turn it into a `trace_*` (table or sink), `trace_many_*` or `eval_*` call."""

    def __init__(self, n: "_Node", staged, fsrc=None):
        t = n.out
        self.kind, self.node_id, self.n = n.kind, t.node_id, t.size
        self.bases = [v.base for v in n.inputs]
        self.bufs = [b.buf for b in self.bases]
        self.views = [_lmn_view(v) for v in n.inputs]
        if fsrc is not None:
            self.op, self.code = "inputs_float", fsrc.code
            self.bufs = [fsrc.tensor.data_ptr() if fsrc.tensor is not None else staged(t.node_id)]
        elif n.kind == int(TraceTableKind.Inputs):
            self.op, self.bufs = "elementwise", [staged(t.node_id)]
        elif n.kind in _REDUCES:
            a = self.bases[0]
            front = int(np.prod(a.shape[:n.axis])) if n.axis else 1
            back = int(np.prod(a.shape[n.axis + 1:])) if n.axis + 1 < len(a.shape) else 1
            self.op, self.shape3, self.maximum = "reduce", (front, a.shape[n.axis], back), n.kind == _REDUCES[1]
        elif _ref_contig(n):
            self.op = "contiguous"
        elif n.kind in _LUT_OF:
            self.op, self.lut = "lut", _LUT_OF[n.kind][0]
        else:
            self.op = "elementwise"
        self.ids = tuple(b.node_id for b in self.bases)

    def pair(self, xs, fill=None):
        """(lhs, rhs) of an elementwise call from the node's zero, one or two inputs"""
        return tuple((list(xs) + [fill, fill])[:2])


def _emit_trace(ctx, c: _Call, lut_dev, lut_ranges, rc_mult, dst):
    """-> `lmn_trace_*` into a table at its row offset, or `lmn_rows_append_*` into a sink (`dst` says which); returns
    the output buffer.  lut_dev: (output column, multiplicities, lo, hi) of the node's LUT."""
    ids = dict(node_id=c.node_id, **dst)
    if c.op == "inputs_float":
        return ctx.trace_inputs_float(c.code, c.bufs[0], c.n, **ids)[1]
    if c.op == "reduce":
        return ctx.trace_sum_reduce(c.bufs[0], *c.shape3, input_id=c.ids[0], maximum=c.maximum, **ids)[1]
    if c.op == "contiguous":
        return ctx.trace_contiguous(c.bufs[0], c.bases[0].size, c.n, input_id=c.ids[0], view=c.views[0], **ids)[1]
    if c.op == "lut":
        col1, mult, lo, hi = lut_dev
        return ctx.trace_lut(c.kind, c.bufs[0], c.n, input_id=c.ids[0], lut_col1=col1, lo=lo, lut_len=hi - lo + 1, mult=mult,
                             view=c.views[0], ranges=lut_ranges, **ids)[1]
    (lhs, rhs), (lv, rv) = c.pair(c.bufs), c.pair(c.views)
    if c.kind == _LESS_THAN:
        return ctx.trace_less_than(lhs, rhs, c.n, input_ids=c.ids, range_check_mult=rc_mult, lhs_view=lv, rhs_view=rv, **ids)[1]
    return ctx.trace_elementwise(c.kind, lhs, rhs, c.n, input_ids=c.ids, input_mults=tuple(-1 for _ in c.ids), lhs_view=lv,
                                 rhs_view=rv, **ids)[1]


def _emit_trace_many(ctx, c: _Call, out_stride: int, lut_dev, lut_ranges, rc_mult, dst):
    """-> `lmn_trace_many_*`; an operand's member stride is its tensor's (0: shared), a graph input's its own"""
    strides = [b.member_stride for b in c.bases] or [out_stride]
    ids = dict(node_id=c.node_id, out_stride=out_stride, **dst)
    if c.op == "inputs_float":
        ctx.trace_many_inputs_float(c.code, c.bufs[0], c.n, src_stride=strides[0], **ids)
    elif c.op == "reduce":
        ctx.trace_many_reduce(c.bufs[0], *c.shape3, input_id=c.ids[0], inp_stride=strides[0], maximum=c.maximum, **ids)
    elif c.op == "contiguous":
        ctx.trace_many_contiguous(c.bufs[0], c.bases[0].size, c.n, input_id=c.ids[0], inp_stride=strides[0], view=c.views[0], **ids)
    elif c.op == "lut":
        col1, mult, mult_stride = lut_dev
        ctx.trace_many_lut(c.kind, c.bufs[0], c.n, input_id=c.ids[0], lut_col1=col1, ranges=lut_ranges, mult=mult,
                           mult_stride=mult_stride, inp_stride=strides[0], view=c.views[0], **ids)
    else:
        (lhs, rhs), (lv, rv), (ls, rs) = c.pair(c.bufs), c.pair(c.views), c.pair(strides, 0)
        lt = c.kind == _LESS_THAN
        ctx.trace_many_elementwise(c.kind, lhs, rhs, c.n, input_ids=c.ids, input_mults=tuple(-1 for _ in c.ids), lhs_stride=ls,
                                   rhs_stride=rs, lhs_view=lv, rhs_view=rv, range_check_mult=rc_mult if lt else None,
                                   range_check_mult_stride=256 if lt else 0, **ids)


def _emit_eval(ctx, c: _Call, lut_col1, lut_ranges, dst):
    """-> `lmn_eval_*`: the values, their range, the refused elements"""
    if c.op == "inputs_float":
        ctx.eval_inputs_float(c.code, c.bufs[0], c.n, **dst)
    elif c.op == "reduce":
        ctx.eval_reduce(c.bufs[0], *c.shape3, maximum=c.maximum, **dst)
    elif c.op == "lut":
        ctx.eval_lut(c.kind, c.bufs[0], c.n, lut_col1, lut_ranges, view=c.views[0], **dst)
    else:       # (the forward pass has one Contiguous: the view rule)
        (lhs, rhs), (lv, rv) = c.pair(c.bufs), c.pair(c.views)
        ctx.eval_elementwise(c.kind, lhs, rhs, c.n, lhs_view=lv, rhs_view=rv, **dst)


class DeviceGraph:
    def __init__(self, ctx: backend.Context):
        self.ctx = ctx
        self.nodes: List[_Node] = []
        self._next_id = 0
        self.luts: Dict[str, tuple] = {}
        self.lut_ranges: Dict[str, list] = {}      # LUTs declared with several ranges (set_lut_ranges)
        self._dry_bufs: list = []                  # device allocations of dry_run_device (release_dry_run)

    def _tensor(self, shape) -> GraphTensor:
        t = GraphTensor(self._next_id, tuple(int(s) for s in shape))
        self._next_id += 1
        return t

    def input(self, values: np.ndarray, per_member: bool = False) -> GraphTensor:
        """A graph input holding Fixed<12> integers (`CopyToStwo`, prim.rs:52-88).  per_member: `gen_trace_many` gives every
        member its own tensor of this shape (through `feeds`); `values` is what `gen_trace` and the dry runs use."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        t = self._tensor(v.shape)
        self.nodes.append(_Node(int(TraceTableKind.Inputs), t, [], host=v, per_member=per_member))
        return t

    def input_float(self, values, per_member: bool = False) -> GraphTensor:
        """A graph input given as floats (`CopyToStwo` with `StwoData::from_f32`, prim.rs:52-101): the conversion to
        Fixed<12> - round to nearest, ties away from zero; NaN, +-Inf and values outside [-(2^30-1), 2^30-1] / 4096 are
        refused elements - happens on the device, in the launch that writes the Inputs rows (`lmn_trace_inputs_float`).
        `values`: a numpy float32 / float16 array, or a torch tensor of float32 / float16 / bfloat16 on the CPU or on the
        context's device.  A device tensor is read where it lies - no staging, no copy (a non-contiguous one is made
        contiguous first) - and the node keeps a reference to it, so its memory outlives the asynchronous launches; it
        must not be written while a `gen_trace` / `gen_trace_many` / `dry_run_device` that reads it is in flight.  The
        context works on a stream of its own: before the first launch of a call that reads torch device memory, torch's
        current stream on that device is synchronised, so what torch has enqueued there so far is visible.  Host
        arrays go up as raw float bits in the call's one staging upload.  per_member: as `input`; the `feeds` of
        `gen_trace_many` are then (n_members, *shape) arrays or tensors of this input's dtype."""
        src = _FloatSource(self.ctx, values, "input_float")
        t = self._tensor(src.shape)
        self.nodes.append(_Node(int(TraceTableKind.Inputs), t, [], per_member=per_member, fsrc=src))
        return t

    def _sync_torch(self, sources) -> None:
        """torch's current stream on the context's device, once, if any of `sources` is torch device memory"""
        if any(s is not None and s.tensor is not None for s in sources):
            import torch
            torch.cuda.current_stream(self.ctx.device).synchronize()

    def constant(self, value: int) -> GraphTensor:
        """`LuminairConstant` (prim.rs:151-200): a one-element tensor, expanded by its consumers."""
        return self.input(np.array([value], dtype=np.int32))

    @staticmethod
    def expand(t, axis: int, size: int) -> TensorView:
        """Insert an expanded dimension of `size` at `axis` (stride 0)."""
        v = _as_view(t)
        return TensorView(v.base, v.shape[:axis] + (int(size),) + v.shape[axis:], v.strides[:axis] + (0,) + v.strides[axis:],
                          v.offset)

    @staticmethod
    def expand_dim(t, axis: int, size: int) -> TensorView:
        """Broadcast an EXISTING dimension of size 1 to `size` (stride 0)."""
        v = _as_view(t)
        if v.shape[axis] != 1:
            raise ValueError("expand_dim broadcasts a dimension of size 1")
        return TensorView(v.base, v.shape[:axis] + (int(size),) + v.shape[axis + 1:],
                          v.strides[:axis] + (0,) + v.strides[axis + 1:], v.offset)

    @staticmethod
    def luminal_expand(t, axis: int, size: int) -> TensorView:
        """`GraphTensor::expand(axis, size)` as the reference's tests use it (crates/graph/src/tests/expansions.rs,
        tests/mod.rs:80-110): a dimension of size 1 at `axis` is broadcast ((2,1).expand(1,3) -> (2,3)); where the
        tensor has no such dimension a new expanded one is inserted ((2,3).expand(2,4) -> (2,3,4)).  Either way the
        element -> buffer index map and the number of repetitions per element are the same."""
        v = _as_view(t)
        if axis < len(v.shape) and v.shape[axis] == 1:
            return DeviceGraph.expand_dim(v, axis, size)
        return DeviceGraph.expand(v, axis, size)

    @staticmethod
    def expand_to(t, shape) -> TensorView:
        """`GraphTensor::expand_to(shape)`: broadcast every dimension of size 1 (leading dimensions are added)."""
        v = _as_view(t)
        shape = tuple(int(d) for d in shape)
        vs, st = (1,) * (len(shape) - len(v.shape)) + v.shape, (0,) * (len(shape) - len(v.shape)) + v.strides
        out = []
        for have, want, stride in zip(vs, shape, st):
            if have == want:
                out.append(stride)
            elif have == 1:
                out.append(0)
            else:
                raise ValueError("expand_to: dimension %d cannot become %d" % (have, want))
        return TensorView(v.base, shape, tuple(out), v.offset)

    @staticmethod
    def slice(t, ranges) -> TensorView:
        """`GraphTensor::slice`: ranges = one (start, stop) per dimension (None = the whole dimension)."""
        v = _as_view(t)
        ranges = list(ranges)
        if len(ranges) > len(v.shape):
            raise ValueError("slice: %d ranges for a %d-dimensional tensor" % (len(ranges), len(v.shape)))
        ranges += [None] * (len(v.shape) - len(ranges))      # missing trailing dimensions are taken whole
        shape, off = [], v.offset
        for d, stride, r in zip(v.shape, v.strides, ranges):
            lo, hi = (0, d) if r is None else r
            if not 0 <= lo < hi <= d:
                raise ValueError("slice out of range")
            shape.append(hi - lo)
            off += lo * stride
        return TensorView(v.base, tuple(shape), v.strides, off)

    @staticmethod
    def permute(t, axes) -> TensorView:
        """`GraphTensor::permute`."""
        v = _as_view(t)
        return TensorView(v.base, tuple(v.shape[a] for a in axes), tuple(v.strides[a] for a in axes), v.offset)

    @staticmethod
    def broadcast_to(t, shape) -> TensorView:
        """View a one-element tensor (a constant) with the given shape."""
        v = _as_view(t)
        if v.base.size != 1:
            raise ValueError("broadcast_to takes a one-element tensor")
        return TensorView(v.base, tuple(int(d) for d in shape), (0,) * len(shape))

    def _consume(self, t) -> TensorView:
        v = _as_view(t)
        v.base.consumers += v.expansion
        return v

    def _binary(self, kind, a, b) -> GraphTensor:
        va, vb = _as_view(a), _as_view(b)
        if va.shape != vb.shape:
            raise ValueError("elementwise operands must have equal (view) shapes: expand / broadcast_to first")
        t = self._tensor(va.shape)
        self.nodes.append(_Node(kind, t, [self._consume(a), self._consume(b)]))
        return t

    def add(self, a, b):
        return self._binary(int(TraceTableKind.Add), a, b)

    def mul(self, a, b):
        return self._binary(int(TraceTableKind.Mul), a, b)

    def _unary(self, kind, a) -> GraphTensor:
        v = self._consume(a)
        t = self._tensor(v.shape)
        self.nodes.append(_Node(kind, t, [v]))
        return t

    def recip(self, a) -> GraphTensor:
        return self._unary(int(TraceTableKind.Recip), a)

    def sqrt(self, a) -> GraphTensor:
        return self._unary(int(TraceTableKind.Sqrt), a)

    def contiguous(self, a) -> GraphTensor:
        """Materialise a view (`LuminairContiguous`, prim.rs:229-301).  A view without expanded dimensions (slice,
        permutation, identity) follows the reference's own row rule - one row per element of the input BUFFER,
        `lmn_trace_contiguous`; a view WITH expanded dimensions consumes the view's element per output row instead
        (the reference's rule cannot balance the logup there)."""
        return self._unary(int(TraceTableKind.Contiguous), a)

    def rem(self, a, b) -> GraphTensor:
        return self._binary(int(TraceTableKind.Rem), a, b)

    def less_than(self, a, b) -> GraphTensor:
        return self._binary(int(TraceTableKind.LessThan), a, b)

    def max_reduce(self, a: GraphTensor, axis: int) -> GraphTensor:
        t = self.sum_reduce(a, axis)
        self.nodes[-1].kind = int(TraceTableKind.MaxReduce)
        return t

    def sum_reduce(self, a: GraphTensor, axis: int) -> GraphTensor:
        if isinstance(a, TensorView):
            raise ValueError("sum_reduce takes a materialised tensor")
        v = self._consume(a)
        shape = a.shape[:axis] + a.shape[axis + 1:]
        t = self._tensor(shape if shape else (1,))
        self.nodes.append(_Node(int(TraceTableKind.SumReduce), t, [v], axis=axis))
        return t

    def set_lut(self, name: str, lo: int, hi: int):
        """Declare the value range of a LUT (what `gen_circuit_settings` derives from a dry run,
        graph.rs:61-159); the columns are generated on the host as the reference does (f64 math)."""
        from . import synthetic
        self.luts[name] = (int(lo), int(hi), synthetic.make_lut(name, int(lo), int(hi)))
        self.lut_ranges.pop(name, None)

    def set_lut_ranges(self, name: str, ranges):
        """A LUT over SEVERAL value ranges - what `gen_circuit_settings` yields when the graph applies the function
        on disjoint input ranges (one padded range per op, coalesced: graph.rs:61-159, 665-691).  `ranges`: ascending,
        disjoint (lo, hi) pairs; columns from `lmn_lut_from_ranges` (`SinPreProcessed::gen_column` and siblings)."""
        rg = [(int(a), int(b)) for a, b in ranges]
        cols = self.ctx.lib.lut_from_ranges(name, rg)
        self.luts[name] = (rg[0][0], rg[-1][1], cols)
        self.lut_ranges[name] = rg

    def _lut_op(self, kind, a) -> GraphTensor:
        v = self._consume(a)
        t = self._tensor(v.shape)
        self.nodes.append(_Node(kind, t, [v]))
        return t

    def sin(self, a):
        return self._lut_op(int(TraceTableKind.Sin), a)

    def exp2(self, a):
        return self._lut_op(int(TraceTableKind.Exp2), a)

    def log2(self, a):
        return self._lut_op(int(TraceTableKind.Log2), a)

    def output(self, t: GraphTensor) -> GraphTensor:
        t.is_output = True
        return t

    def gen_trace(self, columns: bool = False, sinks: Optional[Dict[int, "backend.RowSink"]] = None):
        """Runs every node on the device.  Returns (tables, luts, buffers): tables = [(kind, rows DeviceBuffer,
        n_rows)] in `gen_trace` order (ascending kind) and luts = {name: (col0, col1)} for
        Context.prove_tables(tables, luts); buffers = every device allocation made (free them after proving).
        columns=True: every operator table is a `RowSink` the producers fill column-major (`lmn_rows_append_*`), so the
        proof starts without the transpose of those tables: the table entries are (kind, finished RowSink, n_rows) - the
        lookup-multiplicity and range-check tables stay one-column device buffers - and `buffers` holds the sinks too, so
        freeing it after the proof closes them.  All sinks are finished after the last node has been enqueued; a refused
        element raises the dry run's ValueError.  sinks= the sinks of an earlier call - {kind: RowSink} as
        `sinks_of(buffers)` returns them, or that call's `buffers` - are reset and reused instead of opened (a service
        does not reallocate per pie); a sink that is closed or too small is replaced."""
        if sinks is not None and not columns:
            raise ValueError("gen_trace: sinks= needs columns=True")
        if sinks is not None and not isinstance(sinks, dict):     # an earlier call's buffers, or any collection of sinks
            sinks = {s.kind: s for s in (b.sink if isinstance(b, _SinkLease) else b for b in sinks)
                     if isinstance(s, backend.RowSink)}
        ctx = self.ctx
        K = TraceTableKind
        self.release_dry_run()     # (its slab goes back to the context's cache: the lease below may take it)
        total: Dict[int, int] = {}
        for n in self.nodes:
            total[n.kind] = total.get(n.kind, 0) + _rows_of(n)
        # one allocation for all tables and tensors; the trace calls are stream-ordered, so nothing waits until the tables
        # are proved or a tensor is read back
        st = _Stager()
        for n in self.nodes:
            if n.kind in _LUT_OF and _LUT_OF[n.kind][0] not in self.luts:
                raise ValueError("no LUT for %r: call gen_circuit_settings() (or set_lut / set_lut_ranges) before gen_trace"
                                 % _LUT_OF[n.kind][0])
            st.stage_input(n, n.host, n.fsrc)
        luts_out = {}
        for kind in sorted(total):
            if kind in _LUT_OF:
                name, _ = _LUT_OF[kind]
                lo, hi, (c0, c1) = self.luts[name]
                st.stage(("lut1", name), c1)
                st.stage(("lutm", name), np.zeros(len(c0), dtype=np.uint32))
                luts_out[name] = (c0, c1)
        if _LESS_THAN in total:
            st.stage(("rc",), np.zeros(256, dtype=np.uint32))
        if columns:
            st.stage(("refused",), np.zeros(1, dtype=np.uint32))
        slab = st.lease(ctx, (0 if columns else sum(_al(total[k] * _NCOLS[k] * 4) for k in total)) +
                        sum(_al(n.out.size * 4) for n in self.nodes))
        st.upload(ctx)
        bufs = [slab]
        refused = None
        if columns:
            # one sink per operator table, of exactly the table's rows: the finish has nothing to compact
            tables = {}
            for k in total:
                sink = (sinks or {}).get(k)
                if sink is None or sink.capacity < total[k] or sink.handle is None:
                    sink = ctx.row_sink(k, total[k])
                else:
                    sink.reset()
                tables[k] = sink
                bufs.append(_SinkLease(sink))
            refused = st.dev_of(("refused",))
        else:
            tables = {k: st.carve(total[k] * _NCOLS[k] * 4) for k in total}
        offset = {k: 0 for k in total}
        lut_dev, lut_tables = {}, {}
        for kind in sorted(total):
            if kind in _LUT_OF:
                name, lookup_kind = _LUT_OF[kind]
                lo, hi, (c0, _) = self.luts[name]
                lut_dev[name] = (st.dev_of(("lut1", name)), st.dev_of(("lutm", name)), lo, hi)   # outputs, multiplicities
                lut_tables[lookup_kind] = (lut_dev[name][1], len(c0))
        rc_mult = None
        if _LESS_THAN in total:
            rc_mult = st.dev_of(("rc",))
            lut_tables[int(K.RangeCheckLookup)] = (rc_mult, 256)
        self._sync_torch(n.fsrc for n in self.nodes)
        for n in self.nodes:
            t = n.out
            t.member_stride = 0
            dst = dict(num_consumers=t.consumers, is_final_output=t.is_output, out=st.carve(t.size * 4))
            if columns:
                dst.update(sink=tables[n.kind], refused=refused)
            else:
                dst.update(rows=tables[n.kind], row_offset=offset[n.kind])
            c = _Call(n, lambda node_id: st.dev_of(("in", node_id)), n.fsrc)
            name = getattr(c, "lut", None)
            t.buf = _emit_trace(ctx, c, lut_dev.get(name), self.lut_ranges.get(name), rc_mult, dst)
            offset[n.kind] += _rows_of(n)
        if columns:
            # every node is enqueued: the first finish waits for nearly all of the work, the others find it done.  A sink
            # fails its finish exactly when a producer refused one of its elements; only then the counter is read
            failed = False
            for sink in tables.values():
                try:
                    sink.finish()
                except backend.LuminairBackendError as e:
                    if e.code != backend.ERR_INVALID_ARGUMENT:
                        raise
                    failed = True
            if failed:
                n_refused = int(ctx.download(refused)[0])
                for b in bufs:
                    if not (isinstance(b, _SinkLease) and sinks is not None and b.sink in sinks.values()):
                        b.free()           # (the caller's own sinks stay open: the next call resets them)
                raise _refused_error(n_refused)
        out = [(k, tables[k], total[k]) for k in tables] + [(k, b, n) for k, (b, n) in lut_tables.items()]
        return sorted(out, key=lambda e: e[0]), luts_out, bufs

    @staticmethod
    def sinks_of(buffers) -> Dict[int, "backend.RowSink"]:
        """The sinks among what `gen_trace(columns=True)` returned as buffers, by kind: pass them as `sinks=` to the next
        call - and then free only the other buffers of this one (closing a sink ends its reuse)."""
        return {b.sink.kind: b.sink for b in buffers if isinstance(b, _SinkLease)}

    def gen_trace_many(self, n_members: int, feeds):
        """`gen_trace` for `n_members` pies of this graph at once - the producers in front of `BatchProver.prove_batch`:
        one `lmn_trace_many_*` call (one launch) per node instead of one per node per pie.  `feeds` maps every input tensor
        created with per_member=True to an array of shape (n_members, *shape); all other inputs are shared by the members.
        The slab discipline is `gen_trace`'s: one lease, one staged upload (shared inputs once, per-member inputs packed),
        per kind one region of n_members x total_rows[kind] rows, per node one region of n_members x size output words - or
        `size` words when everything the node reads is shared.  The call ends with ONE download, of the n_members refused
        counters: the only wait, and what orders the producers' stream in front of whoever proves the tables.
        LUT ranges are what the graph declares (set_lut, set_lut_ranges or an earlier gen_circuit_settings): a batch shares
        one settings object.  Returns (pies, luts, bufs, refused): pies[m] = [(kind, DeviceBuffer view, n_rows)] for
        `BatchProver.prove_batch(pies, luts)` (or `Context.prove_tables(pies[m], luts)`), refused[m] = member m's refused
        elements - nothing is raised for them: the prover refuses such a member's pie alone."""
        ctx = self.ctx
        K = TraceTableKind
        n_members = int(n_members)
        if not 1 <= n_members <= backend.TRACE_MANY_MAX:
            raise ValueError("gen_trace_many: 1..%d members" % backend.TRACE_MANY_MAX)
        self.release_dry_run()
        fed = {}
        float_nodes = {n.out.node_id: n for n in self.nodes if n.fsrc is not None}
        for t, arr in (feeds.items() if hasattr(feeds, "items") else feeds):
            if t.node_id in float_nodes:
                fed[t.node_id] = f = _FloatSource(ctx, arr, "gen_trace_many: feeds")
                if f.code != float_nodes[t.node_id].fsrc.code:
                    raise ValueError("gen_trace_many: the feed of input %d has another dtype than the input" % t.node_id)
            else:
                fed[t.node_id] = np.ascontiguousarray(arr, dtype=np.int32)
        total: Dict[int, int] = {}
        varying = set()            # tensors that differ between members: the per-member inputs and what depends on them
        for n in self.nodes:
            total[n.kind] = total.get(n.kind, 0) + _rows_of(n)
            if n.per_member or any(i.base.node_id in varying for i in n.inputs):
                varying.add(n.out.node_id)
            if n.kind in _LUT_OF and _LUT_OF[n.kind][0] not in self.luts:
                raise ValueError("no LUT for %r: call gen_circuit_settings() (or set_lut / set_lut_ranges) before gen_trace_many"
                                 % _LUT_OF[n.kind][0])
            if n.per_member:
                a = fed.get(n.out.node_id)
                if a is None or a.shape != (n_members,) + n.out.shape:
                    raise ValueError("gen_trace_many: feeds must hold an array of shape (n_members, *shape) for input %d"
                                     % n.out.node_id)
        extra = set(fed) - {n.out.node_id for n in self.nodes if n.per_member}
        if extra:
            raise ValueError("gen_trace_many: feeds name tensors that are no per_member inputs: %s" % sorted(extra))
        # what an input node reads: its feed when it is per_member, the graph's own values otherwise
        host_of = lambda n: fed[n.out.node_id] if n.per_member else n.host
        fsrc_of = lambda n: n.fsrc if n.fsrc is None or not n.per_member else fed[n.out.node_id]
        st = _Stager()
        st.stage(("refused",), np.zeros(n_members, dtype=np.uint32))
        for n in self.nodes:
            st.stage_input(n, host_of(n), fsrc_of(n))
        luts_out, lut_dev, lut_rg = {}, {}, {}
        for kind in sorted(total):
            if kind in _LUT_OF:
                name, _ = _LUT_OF[kind]
                lo, hi, (c0, c1) = self.luts[name]
                lut_rg[name] = self.lut_ranges.get(name) or [(lo, hi)]
                st.stage(("lut1", name), c1)
                st.stage(("lutm", name), np.zeros(n_members * len(c0), dtype=np.uint32))
                luts_out[name] = (c0, c1)
        if _LESS_THAN in total:
            st.stage(("rc",), np.zeros(n_members * 256, dtype=np.uint32))
        out_words = lambda n: n.out.size * (n_members if n.out.node_id in varying else 1)
        slab = st.lease(ctx, sum(_al(n_members * total[k] * _NCOLS[k] * 4) for k in total) +
                        sum(_al(out_words(n) * 4) for n in self.nodes))
        st.upload(ctx)
        staged, stage_off = st.staged, st.off
        refused = st.dev_of(("refused",))
        tables = {k: st.carve(n_members * total[k] * _NCOLS[k] * 4) for k in total}
        offset = {k: 0 for k in total}
        lut_len = {name: len(c0) for name, (c0, _) in luts_out.items()}
        for name in luts_out:
            lut_dev[name] = (st.dev_of(("lut1", name)), st.dev_of(("lutm", name)), lut_len[name])
        rc_mult = st.dev_of(("rc",)) if _LESS_THAN in total else None
        self._sync_torch(fsrc_of(n) for n in float_nodes.values())
        for n in self.nodes:
            t = n.out
            t.member_stride = t.size if t.node_id in varying else 0
            t.buf = st.carve(out_words(n) * 4)
            dst = dict(n_members=n_members, num_consumers=t.consumers, is_final_output=t.is_output, rows=tables[n.kind],
                       rows_stride=total[n.kind], row_offset=offset[n.kind], out=t.buf, refused=refused)
            c = _Call(n, lambda node_id: st.dev_of(("in", node_id)), fsrc_of(n))
            name = getattr(c, "lut", None)
            _emit_trace_many(ctx, c, t.member_stride, lut_dev.get(name), lut_rg.get(name), rc_mult, dst)
            offset[n.kind] += _rows_of(n)
        counts = [int(c) for c in ctx.download(refused)[:n_members]]      # the one wait
        pies = []
        for m in range(n_members):
            pie = [(k, tables[k].view(m * total[k] * _NCOLS[k] * 4, total[k] * _NCOLS[k] * 4), total[k]) for k in tables]
            for kind in total:
                if kind in _LUT_OF:
                    name, lookup_kind = _LUT_OF[kind]
                    ln = lut_len[name]
                    off, _ = stage_off[("lutm", name)]
                    pie.append((lookup_kind, staged.view(off + m * ln * 4, ln * 4), ln))
            if int(K.LessThan) in total:
                off, _ = stage_off[("rc",)]
                pie.append((int(K.RangeCheckLookup), staged.view(off + m * 1024, 1024), 256))
            pies.append(sorted(pie, key=lambda e: e[0]))
        return pies, luts_out, [slab], counts

    def read(self, t: GraphTensor, member: Optional[int] = None) -> np.ndarray:
        """The tensor's values.  After `gen_trace_many`: member `member`'s tensor, or the shared tensor of a node that
        depends on no per-member input (for which `member` is ignored)."""
        buf = t.buf
        if t.member_stride:
            if member is None:
                raise ValueError("read: tensor %d differs between members: pass member=" % t.node_id)
            buf = buf.view(int(member) * t.member_stride * 4, t.size * 4)
        return self.ctx.download(buf, np.int32).reshape(t.shape)

    def read_float(self, t: GraphTensor, member: Optional[int] = None, dtype=np.float32, device: bool = False):
        """The tensor's values as floats (`CopyFromStwo`, prim.rs:90-101: `d.to_f64() as f32`): v / 4096 rounded once to
        `dtype`, to nearest even, by `lmn_tensor_to_float` on the device.  dtype: float32, float16 or bfloat16 (numpy or
        torch dtype, or "bfloat16").  Returns a numpy array - for bfloat16, which numpy lacks, its uint16 bit patterns - or,
        with device=True, a torch tensor on the context's device, filled with no host trip and complete when the call
        returns.  `member` as in `read`."""
        code = backend.float_dtype_code(dtype)
        buf = t.buf
        if t.member_stride:
            if member is None:
                raise ValueError("read_float: tensor %d differs between members: pass member=" % t.node_id)
            buf = buf.view(int(member) * t.member_stride * 4, t.size * 4)
        if device:
            import torch
            tdt = {backend.F32: torch.float32, backend.F16: torch.float16, backend.BF16: torch.bfloat16}[code]
            out = torch.empty(t.shape, dtype=tdt, device="cuda:%d" % self.ctx.device)
            # (the allocator may hand out memory that work on torch's stream still uses; the context writes on its own)
            torch.cuda.current_stream(self.ctx.device).synchronize()
            self.ctx.tensor_to_float(code, buf, t.size, dst=out.data_ptr())
            return out
        dst = self.ctx.tensor_to_float(code, buf, t.size)
        try:
            bits = self.ctx.download(dst, np.uint32 if code == backend.F32 else np.uint16)[:t.size]
        finally:
            dst.free()
        return (bits.view(np.float32) if code == backend.F32 else bits.view(np.float16) if code == backend.F16
                else bits).reshape(t.shape)

    # ---- gen_circuit_settings (crates/graph/src/graph.rs:61-159): a HOST dry run, as in the reference
    def _dry_run(self) -> Dict[int, np.ndarray]:
        """Every node's values as Fixed<12> integers, computed on the host with the same integer rules as the device
        kernels (`Operator::process` in the reference: plain CPU execution, no trace)."""
        S = 4096
        fn = {int(TraceTableKind.Sin): np.sin, int(TraceTableKind.Exp2): np.exp2, int(TraceTableKind.Log2): np.log2}
        K = TraceTableKind
        vals: Dict[int, np.ndarray] = {}

        def view(v):
            base = vals[v.base.node_id].reshape(-1)
            idx = np.full(v.shape, v.offset, dtype=np.int64)
            for ax, (d, st) in enumerate(zip(v.shape, v.strides)):
                shp = [1] * len(v.shape)
                shp[ax] = d
                idx = idx + (np.arange(d, dtype=np.int64) * st).reshape(shp)
            return base[idx.reshape(-1)]

        for n in self.nodes:
            k = n.kind
            if n.fsrc is not None:
                out = n.fsrc.fixed().astype(np.int64).reshape(-1)     # (a device-resident input comes down once)
            elif k == int(K.Inputs):
                out = n.host.astype(np.int64).reshape(-1)
            elif k in (int(K.Add), int(K.Mul), int(K.Rem), int(K.LessThan)):
                a, b = view(n.inputs[0]), view(n.inputs[1])
                out = a + b if k == int(K.Add) else (a * b) >> 12 if k == int(K.Mul) else a % b if k == int(K.Rem) \
                    else np.where(a < b, S, 0)
            elif k == int(K.Recip):
                out = (S * S) // view(n.inputs[0])
            elif k == int(K.Sqrt):
                a = view(n.inputs[0])
                out = np.array([int(np.floor(np.sqrt(float(x) * S))) for x in a], dtype=np.int64)
                out = np.where(out * out > a * S, out - 1, out)
                out = np.where((out + 1) * (out + 1) <= a * S, out + 1, out)
            elif k == int(K.Contiguous):
                out = view(n.inputs[0])
            elif k in (int(K.SumReduce), int(K.MaxReduce)):
                a = n.inputs[0].base
                x = np.moveaxis(vals[a.node_id].reshape(a.shape), n.axis, -1).reshape(-1, a.shape[n.axis])
                out = x.sum(axis=1) if k == int(K.SumReduce) else x.max(axis=1)
            elif k in fn:
                out = np.rint(fn[k](view(n.inputs[0]) / S) * S).astype(np.int64)
            else:
                raise ValueError("dry run: kind %d" % k)
            vals[n.out.node_id] = np.asarray(out, dtype=np.int64).reshape(-1)
        return vals

    # ---- the same dry run on the device: the eval forms of the producers (lmn_eval_*), ranges fused into the launches
    def release_dry_run(self) -> None:
        """Give back what `dry_run_device` allocated (`gen_trace` does it too).  The nodes' tensors are gone after it."""
        for b in self._dry_bufs:
            b.free()
        if self._dry_bufs:
            for n in self.nodes:
                n.out.buf = None
        self._dry_bufs = []

    def dry_run_device(self) -> Dict[str, list]:
        """Every node's values computed in HBM by `lmn_eval_*`, in node order, in one slab; every launch leaves the range
        of the buffer it wrote in the node's two-word slot.  At a Sin / Exp2 / Log2 node the two words of its source
        BUFFER come to the host (the one round trip of that node), the padded range is computed as in
        `gen_circuit_settings`, its columns come from `lmn_lut_from_ranges`, and column 1 goes up for `eval_lut` - so
        the dry run's LUT outputs are the ones `gen_trace` reads.  Returns {lut name: [(lo, hi) per node]} and leaves
        every tensor readable (`read`) until `gen_trace` or `release_dry_run`.  Raises ValueError when an element was
        refused (outside the producers' contract: the host dry run divides by zero or goes on with garbage there)."""
        ctx = self.ctx
        self.release_dry_run()
        # staged in one upload: the refused counter (zero) and the range slots, then the graph inputs
        st = _Stager()
        st.stage(("head",), np.zeros(64 + 2 * len(self.nodes), dtype=np.uint32))
        for n in self.nodes:
            st.stage_input(n, n.host, n.fsrc)
        self._dry_bufs = [st.lease(ctx, sum(_al(n.out.size * 4) for n in self.nodes))]
        per_fn: Dict[str, list] = {"sin": [], "exp2": [], "log2": []}
        try:
            st.upload(ctx)
            head = st.dev_of(("head",))
            refused = head.view(0, 4)
            slot = {n.out.node_id: head.view(256 + 8 * i, 8) for i, n in enumerate(self.nodes)}
            self._sync_torch(n.fsrc for n in self.nodes)
            for n in self.nodes:
                t = n.out
                t.buf = st.carve(t.size * 4)
                c = _Call(n, lambda node_id: st.dev_of(("in", node_id)), n.fsrc)
                col1 = rg = None
                if c.op == "lut":
                    lo, hi = (int(w) for w in ctx.download(slot[c.ids[0]], np.int32))   # of the BUFFER, not the view
                    rg = [_padded_lut_range(c.lut, lo, hi)]
                    per_fn[c.lut] += rg
                    col1 = ctx.upload(ctx.lib.lut_from_ranges(c.lut, rg)[1])
                    self._dry_bufs.append(col1)
                _emit_eval(ctx, c, col1, rg, dict(out=t.buf, minmax=slot[t.node_id], refused=refused))
            n_refused = int(ctx.download(refused)[0])
        except Exception:
            self.release_dry_run()
            raise
        if n_refused:
            self.release_dry_run()
            raise _refused_error(n_refused)
        return per_fn

    def gen_circuit_settings(self, device: bool = False):
        """`LuminairGraph::gen_circuit_settings` (crates/graph/src/graph.rs:61-159): dry-run the graph, give every
        Sin / Exp2 / Log2 node the min..max of its source BUFFER padded by 10 % of the span
        (`compute_padded_range_from_srcs` / `buffer_range`, crates/graph/src/utils.rs:44-82), coalesce overlapping or
        adjacent ranges per function (`coalesce_ranges`, graph.rs:665-691), and announce the 8-bit range check when a
        LessThan node exists.  Declares the LUTs on this graph (`set_lut_ranges`) and returns the `CircuitSettings` in
        the reference's own (serialisable) form.  Unpinned: `Fixed::from_f64` of the padded bounds is taken as
        round-to-nearest (numerair is un-vendored); a log2 range whose padding reaches <= 0 is clipped at the smallest
        positive value (the reference would emit LUT rows from log2 of a non-positive number there).
        device=True: the dry run runs on the GPU (`dry_run_device`) - its LUT outputs are the LUT columns' own, and
        `read(t)` returns its tensors until `gen_trace` or `release_dry_run`; the default is the host dry run."""
        from .pie import CircuitSettings, Lookup, LookupLayout, RangeCheckLookup
        if device:
            per_fn = self.dry_run_device()
        else:
            vals = self._dry_run()
            per_fn = {"sin": [], "exp2": [], "log2": []}
            for n in self.nodes:
                if n.kind in _LUT_OF:
                    buf = vals[n.inputs[0].base.node_id]
                    name = _LUT_OF[n.kind][0]
                    per_fn[name].append(_padded_lut_range(name, int(buf.min()), int(buf.max())))
        layouts = {}
        for name, rg in per_fn.items():
            if not rg:
                continue
            rg.sort()
            merged = [list(rg[0])]
            for lo, hi in rg[1:]:
                if lo <= merged[-1][1] + 1:
                    merged[-1][1] = max(merged[-1][1], hi)
                else:
                    merged.append([lo, hi])
            merged = [tuple(r) for r in merged]
            self.set_lut_ranges(name, merged)
            log_size = self.ctx.lib.lut_log_size(merged)
            layouts[name] = Lookup(LookupLayout(merged, log_size), [0] * (1 << log_size))
        rc = RangeCheckLookup([8], 8, [0] * 256) if any(n.kind == int(TraceTableKind.LessThan) for n in self.nodes) else None
        return CircuitSettings(layouts=layouts or None, range_check=rc)

    def fill_multiplicities(self, settings, tables) -> None:
        """What `gen_trace(&mut settings)` leaves in the settings' `AtomicMultiplicityColumn`s: the lookup tables'
        multiplicity columns (downloaded from the device tables `gen_trace` returned)."""
        kinds = {"sin": 4, "exp2": 10, "log2": 12}
        by_kind = {k: (b, n) for k, b, n in tables}
        for name, lk in (settings.layouts or {}).items():
            if kinds[name] in by_kind:
                b, n = by_kind[kinds[name]]
                lk.multiplicities = [int(v) for v in self.ctx.download(b.view(0, n * 4))]
        if settings.range_check is not None and 14 in by_kind:
            b, n = by_kind[14]
            settings.range_check.multiplicities = [int(v) for v in self.ctx.download(b.view(0, n * 4))]
