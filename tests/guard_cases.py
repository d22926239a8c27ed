"""Memory guards for the kernels of the training step's hot path, shared by tests/test_kernels_guard_gpu.py (the case table, on the GPU) and
tests/test_guard_cases_cpu.py (the arena's own logic and the gate's teeth, on CPU tensors).

The property of a case: the same logical operands run twice -- as tight, fresh allocations through the ``ops`` wrapper (the path the fp64 tests hold to their
bands), and as views of an ``Arena`` through ``ops._call`` -- and the two results are EQUAL BITS (or, where the kernel adds with atomics, inside the band of
the entry point's own direct test).  What the arena adds around the same values:

  inputs      at an offset that meets exactly the alignment the header states for the operand (address = align modulo 2 * align), with the row stride asked
              for, and NaN in everything that is not an operand element: a guard of one kernel tile (64 rows of the operand's stride, 256 elements for a
              flat operand) on both sides, the gap columns of a strided operand, the pad rows Tk..Tkr of a row-padded K / V buffer.  An integer operand
              is surrounded by ``INT_POISON``, a value outside its valid range.
  outputs     NaN inside (an element still NaN afterwards was never written), the finite ``SENTINEL`` in guards, gaps and pad rows (a changed bit there is a
              write outside the output).  An accumulating / in-place output starts from given finite contents instead of NaN.
  workspaces  views of exactly the documented size between sentinel guards.

``Arena.report()`` says what happened; ``check_case`` is the gate: guards bit-intact, outputs fully written (or exactly the documented part) and finite,
equal to the baseline -- in this order, so that the first message names the cause and not its consequence."""
import ctypes
import math

import numpy as np
import torch

SENTINEL = 12345.0
INT_POISON = -7                     # key_valid holds 0 / 1
TILE_ROWS, FLAT_GUARD = 64, 256     # guard: rows of a 2-D operand (one 64-row kernel tile) / elements of a flat one
_BASE_ALIGN = 64                    # bytes; the flat buffers start on it, so every offset modulo 2 * align <= 32 is the arena's own choice
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _poison(dtype):
    return float("nan") if dtype.is_floating_point else INT_POISON


def _outside(dtype):
    return SENTINEL if dtype.is_floating_point else INT_POISON


class _Spec:
    def __init__(self, name, role, dtype, shape, ld, align, period, init, written):
        self.name, self.role, self.dtype, self.shape, self.align, self.period, self.init, self.written = name, role, dtype, tuple(shape), align, period, init, written
        self.strided = ld is not None
        if ld is None:                               # contiguous, any rank: one run of numel elements
            self.rows, self.cols, self.ld = 1, int(np.prod(self.shape)), int(np.prod(self.shape))
            self.guard = FLAT_GUARD
        else:
            assert len(self.shape) == 2 and ld >= self.shape[1], (name, shape, ld)
            self.rows, self.cols, self.ld = self.shape[0], self.shape[1], int(ld)
            self.guard = TILE_ROWS * self.ld
        if period is not None:                       # (valid, total) rows per batch item: rows r with r % total >= valid are padding, not operand
            assert ld is not None and self.rows % period[1] == 0 and 0 < period[0] <= period[1], (name, period)
        self.span = (self.rows - 1) * self.ld + self.cols
        self.off = None

    def valid_rows(self):
        r = np.arange(self.rows)
        return r if self.period is None else r[r % self.period[1] < self.period[0]]

    def owned(self):
        """the operand's own elements in its flat buffer: a slice (contiguous operand) or an index array"""
        if not self.strided:
            return slice(self.off, self.off + self.span)
        return (self.off + self.valid_rows()[:, None] * self.ld + np.arange(self.cols)[None, :]).reshape(-1)


class Arena:
    """Named operands of ONE kernel call as views of one flat buffer per dtype.  ``inp`` / ``out`` / ``ws`` declare, ``build`` lays out and fills,
    ``view`` / ``p`` hand the operands to the call, ``report`` reads the result.  Works on any device: its logic is tested on the CPU."""

    def __init__(self, dev):
        self.dev, self.specs, self.flat, self.snap, self._owned, self._built = torch.device(dev), {}, {}, {}, {}, False

    # ---------------------------------------------------------------- declaration
    def _add(self, name, role, dtype, shape, ld, align, period, init=None, written=None):
        assert not self._built and name not in self.specs, name
        self.specs[name] = _Spec(name, role, dtype, shape, ld, max(align, dtype.itemsize), period, init, written)
        return self

    def inp(self, name, data, *, ld=None, align=16, period=None):
        """``data``: the TIGHT operand (valid rows only, contiguous); it is scattered into the view by ``build``."""
        shape = data.shape if period is None else (data.shape[0] // period[0] * period[1], data.shape[1])
        return self._add(name, "in", data.dtype, shape, ld, align, period, init=data)

    def out(self, name, shape, dtype, *, ld=None, align=16, period=None, init=None, written=None):
        """``shape``: the view's full shape (pad rows included).  ``init`` (tight): an accumulating / in-place output starts from it, else NaN and every
        element must be written -- or exactly those of the tight boolean mask ``written`` where the contract leaves the rest alone."""
        return self._add(name, "out", dtype, shape, ld, align, period, init, written)

    def ws(self, name, numel, dtype=torch.float32, *, align=16):
        """A workspace of exactly ``numel`` elements: what the kernel leaves in it is its own business, what it writes around it is not."""
        return self._add(name, "ws", dtype, (numel,), None, align, None)

    # ---------------------------------------------------------------- layout
    def build(self):
        assert not self._built
        by_dtype = {}
        for s in self.specs.values():
            by_dtype.setdefault(s.dtype, []).append(s)
        for dtype, specs in by_dtype.items():
            isz, off = dtype.itemsize, 0
            for s in specs:
                off += s.guard
                off += (s.align // isz - off) % (2 * s.align // isz)       # address = align (mod 2 align), in elements
                s.off = off
                off += s.span + s.guard
            slack = _BASE_ALIGN // isz
            raw = torch.empty(off + slack, dtype=dtype, device=self.dev)
            start = (-raw.data_ptr() % _BASE_ALIGN) // isz
            flat = raw[start:start + off]
            assert flat.data_ptr() % _BASE_ALIGN == 0
            flat.fill_(_outside(dtype))                  # the alignment filler between two operands' guards
            # everything that is not an operand element: poison around inputs, the sentinel around outputs and workspaces
            for s in specs:
                flat[s.off - s.guard:s.off + s.span + s.guard] = _poison(dtype) if s.role == "in" else _outside(dtype)
            self.flat[dtype] = flat
            own = np.zeros(off, dtype=bool)
            for s in specs:
                idx = s.owned()
                assert not own[idx].any(), f"{s.name}: overlaps another operand"
                own[idx] = True
            self._owned[dtype] = own
            for s in specs:
                if s.role == "ws" or (s.role == "out" and s.init is None):
                    self._scatter(s, torch.full((len(s.valid_rows()), s.cols), float("nan"), dtype=dtype, device=self.dev))
                else:
                    self._scatter(s, s.init.to(self.dev).reshape(len(s.valid_rows()), s.cols))
            self.snap[dtype] = flat.clone()
        self._built = True
        for s in self.specs.values():
            a = self.flat[s.dtype].data_ptr() + s.off * s.dtype.itemsize
            assert a % (2 * s.align) == s.align, (s.name, a, s.align)
        return self

    def _sel(self, s):
        idx = s.owned()
        return idx if isinstance(idx, slice) else torch.from_numpy(idx).to(self.dev)

    def _scatter(self, s, tight):
        self.flat[s.dtype][self._sel(s)] = tight.reshape(-1).to(s.dtype)

    # ---------------------------------------------------------------- handing out
    def view(self, name):
        """The operand as the kernel sees it: a 2-D strided view (pad rows included) or the contiguous tensor of the declared shape."""
        s = self.specs[name]
        if not s.strided:
            return self.flat[s.dtype][s.off:s.off + s.span].view(s.shape)
        return torch.as_strided(self.flat[s.dtype], (s.rows, s.cols), (s.ld, 1), s.off)

    def tight(self, name):
        """The operand's own elements as a fresh contiguous tensor: [valid rows, cols], or the declared shape of a contiguous operand."""
        s = self.specs[name]
        t = self.flat[s.dtype][self._sel(s)].clone()
        return t.view(-1, s.cols) if s.strided else t.view(s.shape)

    def ld(self, name):
        return self.specs[name].ld

    def address(self, name):
        s = self.specs[name]
        return self.flat[s.dtype].data_ptr() + s.off * s.dtype.itemsize

    def p(self, name):
        return None if name is None else ctypes.c_void_p(self.address(name))

    def guard_mask(self, dtype):
        """numpy bool over the flat buffer of ``dtype``: True where NO operand owns the element (guards, gap columns, pad rows, alignment filler)."""
        return ~self._owned[dtype]

    # ---------------------------------------------------------------- reading the result
    def report(self):
        """dict(guards=[...], inputs=[...], unwritten={name: n}, stray={name: n}, nonfinite={name: n}).  ``guards``: (dtype, flat index, nearest operand) of
        every element outside all operands whose bits changed; ``inputs``: names of inputs whose own elements changed; ``unwritten``: output elements that
        still hold the NaN prefill though the contract has them written; ``stray``: elements the contract leaves alone that were written; ``nonfinite``:
        written output elements that are not finite."""
        rep = dict(guards=[], inputs=[], unwritten={}, stray={}, nonfinite={})
        for dtype, flat in self.flat.items():
            bits = _BITS[dtype.itemsize]
            changed = (flat.view(bits) != self.snap[dtype].view(bits)).cpu().numpy()
            for i in np.flatnonzero(changed & self.guard_mask(dtype))[:8]:
                near = min((s for s in self.specs.values() if s.dtype == dtype), key=lambda s: 0 if s.off <= i < s.off + s.span else min(abs(i - s.off), abs(i - s.off - s.span + 1)))
                rep["guards"].append((str(dtype), int(i), f"{near.name}{'+' if i >= near.off else ''}{int(i) - near.off}"))
            for s in self.specs.values():
                if s.dtype == dtype and s.role == "in" and changed[s.owned()].any():
                    rep["inputs"].append(s.name)
        for s in self.specs.values():
            if s.role != "out" or not s.dtype.is_floating_point:
                continue
            t = self.tight(s.name).reshape(len(s.valid_rows()), s.cols)
            if s.init is None:
                nan = torch.isnan(t)
                must = torch.ones_like(nan) if s.written is None else s.written.to(self.dev).reshape(nan.shape)
                if int((nan & must).sum()):
                    rep["unwritten"][s.name] = int((nan & must).sum())
                if int((~nan & ~must).sum()):
                    rep["stray"][s.name] = int((~nan & ~must).sum())
                bad = ~torch.isfinite(t) & must & ~nan
            else:
                bad = ~torch.isfinite(t)
            if int(bad.sum()):
                rep["nonfinite"][s.name] = int(bad.sum())
        return rep


class GuardFailure(AssertionError):
    pass


def check_case(tag, arena, baseline, *, band=None, show=True):
    """The gate of one case.  ``baseline``: {output name: the tight-layout result of the same operands}.  ``band(name, got, want)``: called instead of the bit
    comparison for the outputs of a kernel that adds with atomics (it asserts and returns the figure to print).  Order: guards, written, finite, equal."""
    rep = arena.report()
    if rep["guards"]:
        raise GuardFailure(f"{tag}: written outside the operands (dtype, flat index, operand+offset): {rep['guards']}")
    if rep["inputs"]:
        raise GuardFailure(f"{tag}: inputs modified: {rep['inputs']}")
    if rep["unwritten"] or rep["stray"]:
        raise GuardFailure(f"{tag}: output elements that still hold NaN -- never written, or written as NaN because the result depends on bytes that are not an operand -- "
                           f"{rep['unwritten']}; written though the contract leaves them alone {rep['stray']}")
    if rep["nonfinite"]:
        raise GuardFailure(f"{tag}: non-finite output elements {rep['nonfinite']}: the result depends on bytes that are not an operand")
    verdict = []
    for name, want in baseline.items():
        got = arena.tight(name).reshape(want.shape)
        s = arena.specs[name]
        if s.written is not None:       # the part the contract leaves alone holds the prefill on one side and whatever the allocator left on the other
            m = s.written.to(got.device).reshape(want.shape)
            got, want = got[m], want.to(got.device)[m]
        if band is not None:
            verdict.append(f"{name} {band(name, got, want.to(got.device))}")
        elif not torch.equal(got, want.to(got.device)):
            diff = (got.double() - want.to(got.device).double()).abs()
            raise GuardFailure(f"{tag}: {name} differs from the tight-layout baseline in {int((got != want.to(got.device)).sum())} of {got.numel()} elements, max |diff| {float(diff.max()):.3e}")
    if show:
        print(f"[guard] {tag}: guards intact / fully written / {'; '.join(verdict) if band is not None else 'bit-equal'}")
    return rep


# ============================================================================= geometry restated from the sources (the library has no query for it)
def gn_fused_geometry(C, HW, G, maxv):
    """csrc/norm.hip gn_fused_geometry: vectors per thread ``nv`` of the single-launch GroupNorm, or None where it does not apply."""
    cg = C // G
    if cg < 8:
        return None
    CB = cg
    while CB & 7:
        CB += cg
    if C % CB or CB // cg > 4 or CB // 8 > 16:
        return None
    rpb = 256 // (CB // 8)
    nv = (HW + rpb - 1) // rpb
    return nv if nv <= maxv else None


def gn_chunk_rows(C, HW):
    """csrc/norm.hip gn_geometry: (rows per chunk, chunks) of the two-launch form (GN_MAX_CHUNKS = 64)."""
    V = C // 8
    rpb = 1 if V >= 256 else 256 // V
    n = (HW + rpb - 1) // rpb if HW < 64 * rpb else 64
    rows = (HW + n - 1) // n
    return rows, (HW + rows - 1) // rows


def gn_fwd_branch(C, HW, G):
    nv = gn_fused_geometry(C, HW, G, 24)
    return "two-launch" if nv is None else "fused<8>" if nv <= 8 else "fused<24>"


def gn_bwd_branch(C, HW, G):
    return "two-launch" if gn_fused_geometry(C, HW, G, 12) is None else "fused"


def wgrad_rp(R):
    return 8 if R <= 8 else 16 if R <= 16 else 32 if R <= 32 else 64


def wgrad_scratch(M, N, R, ldx):
    """csrc/lora.hip fd_lora_wgrad: (vectorised arm?, floats of partials the call writes when the scratch does not force fewer splits)."""
    RP = wgrad_rp(R)
    vec = (RP == 8 and N % 8 == 0 and ldx % 8 == 0) or (RP == 16 and N % 4 == 0 and ldx % 4 == 0)
    cpb = (320 if RP == 8 else 160) if vec else 64
    ncb = (N + cpb - 1) // cpb
    nsplit = min((768 + ncb - 1) // ncb, (M + 63) // 64)
    return vec, nsplit * N * RP


def wgrad_multi_scratch(problems, RP):
    """csrc/lora.hip fd_lora_wgrad_multi: floats of partials for ``problems`` = [(M, N)] of one padded rank (both arms, no forced halving)."""
    work = float(sum(M * N for M, N in problems))
    total = 0
    for M, N in problems:
        if RP <= 16:
            ncb = (N + (320 if RP == 8 else 160) - 1) // (320 if RP == 8 else 160)
            nsplit = min(max(int(1536.0 * (M * N / work) / ncb + 0.5), 1), (M + 63) // 64)
            rows = (-(-M // nsplit) + 5) // 6 * 6
        else:
            ncb = (N + 319) // 320
            nsplit = max(min(int(512.0 * (M * N / work) / ncb + 0.5), (M + 255) // 256), 1)
            rows = (-(-M // nsplit) + 31) // 32 * 32
        total += -(-M // rows) * N * RP
    return total


def fwd_two_blocks(d, Tq, Tk, BH):
    """csrc/attn.hip fwd_qb: does the forward give a wave two 32-query blocks (256-row workgroups)?"""
    return d <= 64 and Tq >= 2048 and Tk >= 2048 and BH * ((Tq + 255) // 256) >= 128


LN_ROWS_PER_WORKGROUP = {1: 16, 2: 16, 4: 8}        # csrc/norm.hip launch_layernorm: 4 waves x R rows, R = 4 / 4 / 2 for MAXV = 1 / 2 / 4


def ln_maxv(C):
    return 1 if C <= 512 else 2 if C <= 1024 else 4


# ============================================================================= bookkeeping
# entry point -> the test of tests/test_kernels_guard_gpu.py that runs it inside an arena
GUARD_TABLE = {
    "fd_attn_fwd": "test_attention", "fd_attn_bwd_dq": "test_attention", "fd_attn_bwd_dkdv": "test_attention", "fd_attn_bwd_prep": "test_attn_bwd_prep_and_sum_slabs",
    "fd_sum_slabs": "test_attn_bwd_prep_and_sum_slabs", "fd_cross_attn_block": "test_cross_attn_block", "fd_small_attn_fwd": "test_small_attn",
    "fd_small_attn_bwd": "test_small_attn", "fd_groupnorm_fwd": "test_groupnorm", "fd_groupnorm_bwd": "test_groupnorm",
    "fd_groupnorm_fwd_stats_p": "test_groupnorm_from_statistics", "fd_groupnorm_fwd_stats": "test_groupnorm_from_statistics",
    "fd_layernorm_fwd": "test_layernorm", "fd_layernorm_bwd": "test_layernorm",
    "fd_geglu_fwd": "test_geglu", "fd_geglu_bwd": "test_geglu", "fd_geglu_bwd_interleaved": "test_geglu",
    "fd_act_fwd": "test_flat_elementwise", "fd_act_bwd": "test_flat_elementwise", "fd_add": "test_flat_elementwise",
    "fd_cast_f32_to_f16": "test_flat_elementwise", "fd_cast_f16_to_f32": "test_flat_elementwise",
    "fd_copy_cols": "test_strided_layout_kernels", "fd_transpose_btc": "test_strided_layout_kernels", "fd_downsum2x2": "test_strided_layout_kernels",
    "fd_nhwc_to_nchw": "test_strided_layout_kernels", "fd_clamp_bwd": "test_strided_layout_kernels",
    "fd_softmax_rows": "test_softmax_rows", "fd_softmax_rows_bwd": "test_softmax_rows",
    "fd_lora_wgrad": "test_lora_wgrad", "fd_lora_wgrad_multi": "test_lora_wgrad_multi",
    "fd_cfg_dpm_step": "test_scheduler_and_optimizer", "fd_grad_finite_scale": "test_scheduler_and_optimizer", "fd_adamw_ema": "test_scheduler_and_optimizer",
}
# entry points whose direct tests already run them as views of a guarded buffer: (test module, test name)
ALREADY_GUARDED = {
    "fd_gemm": ("test_kernels_sharp_gpu.py", "test_gemm_case"),
    "fd_cosine_logits_fwd": ("test_kernels_cosinehead_gpu.py", "test_cosine_head_table_against_fp64"),
    "fd_cosine_logits_bwd": ("test_kernels_cosinehead_gpu.py", "test_cosine_head_table_against_fp64"),
    "fd_lora_merge_multi": ("test_kernels_loramerge_gpu.py", "test_table_against_fp64"),
    "fd_lora_refresh_multi": ("test_kernels_edges_gpu.py", "test_lora_refresh_multi_bit_exact"),
    "fd_bank_norms": ("test_kernels_banknorms_gpu.py", "test_padding_between_tensors_is_never_read"),
}
# the remaining gap: image-side and evaluator entry points, held to fp64 on tight allocations only
NOT_YET_GUARDED = {
    "fd_conv_small_cin": "direct convolution of the tiny channel counts (conv_in, classifier stem)",
    "fd_conv_small_cin_bwd": "its input gradient",
    "fd_dwconv_fwd": "depthwise convolution of the classifier",
    "fd_dwconv_bwd": "its input gradient",
    "fd_avgpool_hw": "squeeze-excite pooling",
    "fd_avgpool_hw_bwd": "its backward",
    "fd_scale_channels": "squeeze-excite scaling",
    "fd_scale_channels_bwd": "its backward",
    "fd_crop_resize_fwd": "face crop + bilinear resize",
    "fd_crop_resize_bwd": "its backward (accumulates into the image gradient)",
    "fd_crop_resize_u8_fwd": "the same from uint8 images (offline evaluator)",
    "fd_warp_affine_fwd": "landmark alignment warp",
    "fd_warp_affine_bwd": "its backward (fixed-order gather)",
    "fd_warp_affine_u8_fwd": "the same from uint8 images (offline evaluator)",
    "fd_patchify_fwd": "ViT patch-embedding input",
    "fd_patchify_bwd": "its backward",
    "fd_rect_scale": "gradient hook of the face rectangle (in place)",
    "fd_ot_assign_sum": "Monte-Carlo transport solves",
    "fd_ot_expected_targets": "exact-enumeration transport targets",
    "fd_eval_tally": "validation counts",
    "fd_eval_grid_u8": "annotated grid painter",
    "fd_eval_grid_attrs_u8": "annotated grid painter, several attributes, uint8 images",
    "fd_eval_grid_attrs": "annotated grid painter, several attributes, training images",
    "fd_eval_grid_labels_u8": "index labels of the grids (in place)",
}


# ============================================================================= torch stand-ins of kernels, right and subtly wrong (tests/test_guard_cases_cpu.py)
def standin_attention(q, k, v, o, H, Tq, Tk, Tkr, fault=None):
    """softmax(q k^T / sqrt(d)) v over VIEWS as fd_attn_fwd takes them (k, v: [Bk * Tkr, C] with pad rows), fp32 math, one batch item per Bk.
    fault "pad_keys": rows Tk..Tkr count as keys;  "pad_v_rows": the probabilities of the pad rows are exactly 0 but their V rows are multiplied in."""
    C = q.shape[1]
    d, B = C // H, q.shape[0] // Tq
    for b in range(B):
        for h in range(H):
            qq = q[b * Tq:(b + 1) * Tq, h * d:(h + 1) * d].float()
            nk = Tkr if fault else Tk
            kk, vv = (t[b * Tkr:b * Tkr + nk, h * d:(h + 1) * d].float() for t in (k, v))
            s = qq @ kk.t() * d ** -0.5
            if fault == "pad_v_rows":
                s[:, Tk:] = -math.inf
            o[b * Tq:(b + 1) * Tq, h * d:(h + 1) * d] = (torch.softmax(s, -1) @ vv).to(o.dtype)


def standin_layernorm(x, y, M, R=None):
    """LayerNorm without affine over the first M rows of x into y; ``R``: a kernel that writes whole groups of R rows (ceil(M / R) * R of them)."""
    rows = M if R is None else -(-M // R) * R
    flat_y = y.as_strided((rows, y.shape[1]), y.stride(), y.storage_offset())
    flat_x = x.as_strided((rows, x.shape[1]), x.stride(), x.storage_offset()).float()
    flat_x = torch.nan_to_num(flat_x, nan=0.0)
    flat_y.copy_(torch.nn.functional.layer_norm(flat_x, (x.shape[1],)).to(y.dtype))


def standin_scale(x, y, n, round_up=False):
    """y[:n] = 2 x[:n]; ``round_up``: a vector body that rounds n up to a multiple of 8."""
    m = -(-n // 8) * 8 if round_up else n
    xs, ys = x.as_strided((m,), (1,), x.storage_offset()), y.as_strided((m,), (1,), y.storage_offset())
    ys.copy_((xs.float() * 2).to(y.dtype))


def standin_groupnorm_stats(x, stats, scratch, B, G, slots, extra=0):
    """Per (sample, group) sums of x [B, G, n] through ``scratch`` [B * slots * G * 2 floats]; ``extra``: floats written behind the documented size."""
    n = B * slots * G * 2 + extra
    sc = scratch.as_strided((n,), (1,), scratch.storage_offset())
    sc.fill_(0.0)
    sc[:B * G * 2].copy_(torch.stack([x.float().sum(-1), (x.float() ** 2).sum(-1)], -1).reshape(-1))
    stats.copy_(sc[:B * G * 2].view(B, G, 2))
