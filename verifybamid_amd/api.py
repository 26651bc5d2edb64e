"""Thin Python marshalling over the C-ABI (include/vb2_abi.h).

Names follow the reference's domain: a *panel* (UD, mu, bed markers), a *pileup*
(bases/quals per marker), a likelihood *context* (the data ComputeMixLLKs sees),
an *estimate* (alpha, PCs, llk1, llk0).  All compute happens in libvb2.so on the
GPU; nothing here evaluates a likelihood.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _abi


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class PileupData:
    """Host arrays in the shape of vb2_input: panel-ordered markers, marker i owning
    bases/quals[read_off[i]:read_off[i+1]] (empty = absent from the pileup)."""
    num_pc: int
    ud: np.ndarray                  # [M, k] f64
    means: np.ndarray               # [M] f64
    read_off: np.ndarray            # [M+1] i64
    bases: np.ndarray               # [R] u8
    quals: np.ndarray               # [R] u8
    alt_base: np.ndarray            # [M] u8
    known_af: np.ndarray | None = None
    avg_depth: float = 0.0
    sd_depth: float = 0.0
    sanity_disabled: bool = True
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.ud = np.ascontiguousarray(self.ud, dtype=np.float64).reshape(-1, self.num_pc)
        self.means = np.ascontiguousarray(self.means, dtype=np.float64)
        self.read_off = np.ascontiguousarray(self.read_off, dtype=np.int64)
        self.bases = np.ascontiguousarray(self.bases, dtype=np.uint8)
        self.quals = np.ascontiguousarray(self.quals, dtype=np.uint8)
        self.alt_base = np.ascontiguousarray(self.alt_base, dtype=np.uint8)
        if self.known_af is not None:
            self.known_af = np.ascontiguousarray(self.known_af, dtype=np.float64)

    @property
    def num_marker(self):
        return int(self.read_off.shape[0] - 1)

    @property
    def num_read(self):
        return int(self.read_off[-1] - self.read_off[0])

    def as_input(self):
        return _abi.Input(self.num_marker, self.num_pc, _p(self.ud), _p(self.means),
                          _p(self.read_off), _p(self.bases), _p(self.quals), _p(self.alt_base),
                          _p(self.known_af), float(self.avg_depth), float(self.sd_depth),
                          int(bool(self.sanity_disabled)), 0)

    def shard_range(self, rank, world):
        """Markers [lo, hi) of shard `rank` of `world` -- the library's own partition (vb2_shard_range)."""
        inp = self.as_input()
        lo, hi = C.c_int32(), C.c_int32()
        _abi.check(_abi.lib().vb2_shard_range(C.byref(inp), int(rank), int(world), C.byref(lo), C.byref(hi)),
                   "vb2_shard_range")
        return lo.value, hi.value

    def shard(self, rank, world):
        """Contiguous marker range holding ~1/world of the READS (balance on R, not M:
        SURVEY 8e).  The depth filter statistics stay global."""
        if world <= 1:
            return self
        lo, hi = self.shard_range(rank, world)
        b, e = int(self.read_off[lo]), int(self.read_off[hi])
        return PileupData(self.num_pc, self.ud[lo:hi], self.means[lo:hi],
                          self.read_off[lo:hi + 1] - b, self.bases[b:e], self.quals[b:e],
                          self.alt_base[lo:hi],
                          None if self.known_af is None else self.known_af[lo:hi],
                          self.avg_depth, self.sd_depth, self.sanity_disabled,
                          dict(self.meta, shard=(rank, world), marker_range=(lo, hi)))

    @staticmethod
    def from_files(svd_prefix, pileup_path, num_pc=2, disable_sanity=True, known_af_path=None):
        """Panel + pileup readers of the library (vb2_flat_load), copied into numpy."""
        L = _abi.lib()
        args, keep = _run_args(svd_prefix, pileup_path, num_pc, disable_sanity, known_af_path, None)
        h = C.c_void_p()
        rc = L.vb2_flat_load(C.byref(args), C.byref(h))
        if rc not in (_abi.VB2_OK, _abi.VB2_ERR_SANITY) or not h:
            _abi.check(rc, "vb2_flat_load")
        try:
            inp = L.vb2_flat_input(h).contents
            M, k = inp.num_marker, inp.num_pc
            off = np.ctypeslib.as_array(C.cast(inp.read_off, C.POINTER(C.c_int64)), (M + 1,)).copy()
            R = int(off[-1])

            def arr(ptr, ctype, n, dt):
                if not ptr or n == 0:
                    return np.zeros(n, dtype=dt)
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).astype(dt, copy=True)
            st = _abi.RunResult()
            L.vb2_flat_stats(h, C.byref(st))
            return PileupData(
                k, arr(inp.ud, C.c_double, M * k, np.float64), arr(inp.means, C.c_double, M, np.float64),
                off, arr(inp.bases, C.c_uint8, R, np.uint8), arr(inp.quals, C.c_uint8, R, np.uint8),
                arr(inp.alt_base, C.c_uint8, M, np.uint8),
                arr(inp.known_af, C.c_double, M, np.float64) if inp.known_af else None,
                inp.avg_depth, inp.sd_depth, bool(inp.sanity_disabled),
                dict(num_site=st.num_site, num_bases=st.num_bases, sanity_ok=(rc == _abi.VB2_OK)))
        finally:
            L.vb2_flat_free(h)


def _model(within_ancestry=False, fix_pc=None, fix_alpha=None, known_af=False, epsilon=1e-8,
           verbose=False):
    fpc = None if fix_pc is None else np.ascontiguousarray(fix_pc, dtype=np.float64)
    m = _abi.Model(int(not within_ancestry), int(fix_pc is not None),
                   int(fix_pc is None and fix_alpha is not None), int(bool(known_af)),
                   float(fix_alpha if fix_alpha is not None else 0.0), _p(fpc), float(epsilon),
                   int(bool(verbose)), 0)
    return m, fpc


def _run_args(svd_prefix, pileup_path, num_pc, disable_sanity, known_af_path, output_prefix,
              device=-1, output_pileup=False, devices=None, num_start=1, seed=0, line_search=False, **model_kw):
    m, keep = _model(known_af=known_af_path is not None, **model_kw)
    enc = lambda s: None if s is None else str(s).encode()
    devs = None
    if devices is not None and len(devices) > 0:
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    args = _abi.RunArgs(enc(svd_prefix + ".UD"), enc(svd_prefix + ".mu"), enc(svd_prefix + ".bed"),
                        enc(pileup_path), enc(known_af_path), enc(output_prefix), int(num_pc),
                        int(bool(disable_sanity)), int(bool(output_pileup)), int(device), m,
                        devs, 0 if devs is None else len(devices), 0, None, None,
                        _abi.SearchOpts(int(num_start), int(seed), 0.0, 1 if line_search else 0, 0))
    return args, (keep, devs)


_CI_NAMES = {1: "ContaminatingSample.PC", 2: "IntendedSample.PC", 3: "PC"}


def _interval_dict(ci):
    rows = []
    for r in range(ci.num_row):
        kind = ci.row_kind[r]
        name = "FREEMIX" if kind == 0 else _CI_NAMES[kind] + str(ci.row_pc[r])
        method = ("profile" if ci.alpha_free else "fixed") if kind == 0 else "wald"
        rows.append(dict(param=name, estimate=ci.row_est[r], stderr=ci.row_se[r], lo=ci.row_lo[r], hi=ci.row_hi[r],
                         method=method))
    return dict(freemix=ci.freemix, freemix_se=ci.freemix_se, lo=ci.lo, hi=ci.hi, llk_max=ci.llk_max,
                llk_lo=ci.llk_lo, llk_hi=ci.llk_hi, alpha_free=bool(ci.alpha_free), num_free=int(ci.num_free),
                pos_def=bool(ci.pos_def), rows=rows, num_launch=int(ci.num_launch), num_profile=int(ci.num_profile))


def _estimate_dict(est, k):
    return dict(alpha=est.alpha, llk1=est.llk1, llk0=est.llk0,
                pc=np.array(est.pc[:k]), pc2=np.array(est.pc2[:k]),
                num_eval=int(est.num_eval), num_launch_point=int(est.num_launch_point),
                converged=bool(est.converged))


def _err_table(err_table):
    e = np.ascontiguousarray(np.asarray(err_table, dtype=np.float64).reshape(-1))
    if e.shape != (_abi.VB2_ERR_NUM_QUAL,):
        raise ValueError("an error table has %d entries, one per clamped quality" % _abi.VB2_ERR_NUM_QUAL)
    return e


def read_err_table(path):
    """vb2_err_table_read: (table [94], the number of qualities the file lists) of a file in .ErrorRates format; the
    qualities it does not list are nominal.  No device."""
    table, taken = np.zeros(_abi.VB2_ERR_NUM_QUAL), C.c_int32(0)
    _abi.check(_abi.lib().vb2_err_table_read(str(path).encode(), _p(table), C.byref(taken)), "vb2_err_table_read")
    return table, int(taken.value)


def _table_of(error_table):
    """error_table= of run_files / run_cohort_files: a path in .ErrorRates format, or the 94 rates."""
    if isinstance(error_table, (str, bytes)) or hasattr(error_table, "__fspath__"):
        return read_err_table(error_table)[0]
    return _err_table(error_table)


def nominal_err_table():
    """The reference's pErr per clamped quality 0..93, pow(10.0, q / -10.0) (ContaminationEstimator.h:65-74)."""
    import math
    return np.array([math.pow(10.0, q / -10.0) for q in range(_abi.VB2_ERR_NUM_QUAL)])


class _TraceBuf:
    def __init__(self, capacity, k):
        self.bufs = dict(alpha=np.zeros(capacity), pc1=np.zeros((capacity, k)),
                         pc2=np.zeros((capacity, k)), llk=np.zeros(capacity))
        self.c = _abi.Trace(capacity, 0, _p(self.bufs["alpha"]), _p(self.bufs["pc1"]),
                            _p(self.bufs["pc2"]), _p(self.bufs["llk"]))
        self.capacity = capacity

    def result(self):
        n = int(min(self.c.count, self.capacity))
        return {k: v[:n] for k, v in self.bufs.items()}, int(self.c.count)


class LikelihoodContext:
    """vb2_ctx: the pileup + panel resident in HBM, ready for batched evaluation."""

    def __init__(self, data: PileupData, device=-1, stream=None, cohort_layout=False, err_table=None):
        """err_table: [94] error rates per clamped quality in place of 10^(-q/10) (vb2_ctx_create_ex)."""
        self._lib = _abi.lib()
        self.data = data
        self.num_pc = data.num_pc
        inp = data.as_input()
        opt = _abi.Options(int(device), 1 if cohort_layout else 0,      # VB2_OPT_COHORT_LAYOUT
                           C.c_void_p(stream) if stream else None)
        h = C.c_void_p()
        if err_table is None:
            _abi.check(self._lib.vb2_ctx_create(C.byref(inp), C.byref(opt), C.byref(h)), "vb2_ctx_create")
        else:
            e = _err_table(err_table)
            _abi.check(self._lib.vb2_ctx_create_ex(C.byref(inp), C.byref(opt), _p(e), C.byref(h)), "vb2_ctx_create_ex")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        i = _abi.Info()
        _abi.check(self._lib.vb2_ctx_info(self._h, C.byref(i)), "vb2_ctx_info")
        d = {name: getattr(i, name) for name, _ in _abi.Info._fields_}
        d["device_name"] = i.device_name.decode()
        d["arch"] = i.arch.decode()
        return d

    def llk(self, pc1, pc2, alpha):
        """+LLK for B points (ComputeMixLLKs, batched).  pc1/pc2: [B,k] (or [k]); alpha: [B]."""
        pc1 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc1, dtype=np.float64)))
        pc2 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc2, dtype=np.float64)))
        alpha = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)))
        B = alpha.shape[0]
        assert pc1.shape == (B, self.num_pc) and pc2.shape == (B, self.num_pc)
        out = np.zeros(B)
        _abi.check(self._lib.vb2_llk_eval_batch(self._h, B, _p(pc1), _p(pc2), _p(alpha), _p(out)),
                   "vb2_llk_eval_batch")
        return out

    def derivatives(self, pc1, pc2, alpha):
        """LLK, gradient and Hessian at B points (vb2_llk_derivs_batch), with respect to (pc1[0..k), pc2[0..k), alpha).
        Returns (llk [B], grad [B, 2k+1], hess [B, 2k+1, 2k+1]).  At alpha 0 or 1 the alpha entries are not defined."""
        pc1 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc1, dtype=np.float64)))
        pc2 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc2, dtype=np.float64)))
        alpha = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)))
        B = alpha.shape[0]
        assert pc1.shape == (B, self.num_pc) and pc2.shape == (B, self.num_pc)
        n = 2 * self.num_pc + 1
        llk, grad, hess = np.zeros(B), np.zeros((B, n)), np.zeros((B, n, n))
        _abi.check(self._lib.vb2_llk_derivs_batch(self._h, B, _p(pc1), _p(pc2), _p(alpha), _p(llk), _p(grad), _p(hess)),
                   "vb2_llk_derivs_batch")
        return llk, grad, hess

    def marginals(self, pc1, pc2, alpha, related=False):
        """Per marker, in panel order, at ONE point (vb2_ctx_marginals): the contaminant-genotype likelihood relative to a
        random contaminant c [M, 3], the posterior of the sample's own genotype q [M, 3] and log L [M]; zeros for the
        markers the sample does not count.  g1 (c) is the alpha-fraction component, g2 (q) the other.
        related: (c, q, log L, h, t) -- also the own-genotype likelihood relative to a random individual h [M, 3] and the
        genotype distribution of a relative sharing one allele by descent t [M, 3] (vb2_ctx_marginals_related)."""
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(-1))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(-1))
        assert pc1.shape == (self.num_pc,) and pc2.shape == (self.num_pc,)
        M = self.data.num_marker
        c, q, ll = np.zeros((M, 3)), np.zeros((M, 3)), np.zeros(M)
        _abi.check(self._lib.vb2_ctx_marginals(self._h, _p(pc1), _p(pc2), float(alpha), _p(c), _p(q), _p(ll)),
                   "vb2_ctx_marginals")
        if related:
            h, t = np.zeros((M, 3)), np.zeros((M, 3))
            _abi.check(self._lib.vb2_ctx_marginals_related(self._h, _p(pc1), _p(pc2), float(alpha), _p(h), _p(t)),
                       "vb2_ctx_marginals_related")
            return c, q, ll, h, t
        return c, q, ll

    def interval(self, estimate, **model_kw):
        """95% confidence interval for FREEMIX and standard errors at an estimate of optimize(**model_kw) on this context
        (vb2_ctx_interval): a dict with freemix, freemix_se, lo, hi, llk_max, llk_lo, llk_hi, pos_def and the .CI rows."""
        m, keep = _model(known_af=self.data.known_af is not None, **model_kw)
        est = _abi.Estimate()
        est.alpha, est.llk1, est.llk0 = estimate["alpha"], estimate["llk1"], estimate.get("llk0", 0.0)
        for j in range(self.num_pc):
            est.pc[j] = float(estimate["pc"][j])
            est.pc2[j] = float(estimate["pc2"][j])
        est.converged = int(bool(estimate.get("converged", True)))
        ci = _abi.Interval()
        _abi.check(self._lib.vb2_ctx_interval(self._h, C.byref(m), C.byref(est), C.byref(ci)), "vb2_ctx_interval")
        return _interval_dict(ci)

    def llk_device(self, points_ptr, out_ptr, num_point, stream=None):
        """Enqueue an evaluation on device pointers (rows = pc1|pc2|alpha); no host sync."""
        _abi.check(self._lib.vb2_llk_eval_batch_device(self._h, int(num_point), C.c_void_p(points_ptr),
                                                       C.c_void_p(out_ptr),
                                                       C.c_void_p(stream) if stream else None),
                   "vb2_llk_eval_batch_device")

    def search(self):
        """Context manager around a series of dependent llk() calls (a search driven by the
        caller): vb2_ctx_search_begin / vb2_ctx_search_end."""
        ctx = self

        class _Search:
            def __enter__(self_inner):
                _abi.check(ctx._lib.vb2_ctx_search_begin(ctx._h), "vb2_ctx_search_begin")
                return ctx

            def __exit__(self_inner, *exc):
                ctx._lib.vb2_ctx_search_end(ctx._h)
                return False

        return _Search()

    def optimize(self, trace_capacity=0, **model_kw):
        """OptimizeLLK on this context.  model_kw: within_ancestry, fix_pc, fix_alpha, epsilon..."""
        m, keep = _model(known_af=self.data.known_af is not None, **model_kw)
        est = _abi.Estimate()
        tb = _TraceBuf(trace_capacity, self.num_pc) if trace_capacity else None
        _abi.check(self._lib.vb2_ctx_optimize_llk(self._h, C.byref(m), C.byref(est),
                                                  C.byref(tb.c) if tb else None),
                   "vb2_ctx_optimize_llk")
        out = _estimate_dict(est, self.num_pc)
        if tb:
            out["trace"], out["trace_count"] = tb.result()
        return out


    def optimize_ex(self, num_start=1, seed=0, start_sd=0.0, line_search=False, **model_kw):
        """Optimiser variants (vb2_ctx_optimize_llk_ex): num_start searches from seeded starting
        points in lock-step (start 0 = the reference's), and / or Brent's line search for the
        one-parameter models.  Returns (best, all): best has "start" = index of the winning run."""
        m, keep = _model(known_af=self.data.known_af is not None, **model_kw)
        n = max(1, int(num_start))
        opts = _abi.SearchOpts(n, int(seed), float(start_sd), 1 if line_search else 0, 0)
        best = _abi.Estimate()
        every = (_abi.Estimate * n)()
        _abi.check(self._lib.vb2_ctx_optimize_llk_ex(self._h, C.byref(m), C.byref(opts), C.byref(best),
                                                     C.cast(every, C.c_void_p)),
                   "vb2_ctx_optimize_llk_ex")
        out = _estimate_dict(best, self.num_pc)
        out["start"] = int(best.reserved)
        return out, [_estimate_dict(every[i], self.num_pc) for i in range(n)]


def _estimate_struct(estimate, k):
    est = _abi.Estimate()
    est.alpha, est.llk1, est.llk0 = estimate["alpha"], estimate.get("llk1", 0.0), estimate.get("llk0", 0.0)
    for j in range(k):
        est.pc[j] = float(estimate["pc"][j])
        est.pc2[j] = float(estimate["pc2"][j])
    est.converged = int(bool(estimate.get("converged", True)))
    return est


class SourceSet:
    """vb2_source_set: the genotype marginals of a cohort's samples (float32, 24 bytes per marker and sample, on one
    device) and every pair's source score S(target, candidate): the log-likelihood ratio of "the target's contaminant
    carries the candidate's genotypes" against "a random individual of the target's fitted contaminant ancestry".
    planes: SourceSet.SOURCE (c, q: scores()), SourceSet.RELATED (q, h, t: relations()) or both; 12 bytes per marker and
    sample for each of c, q, h, t the set holds."""

    SOURCE, RELATED = _abi.VB2_SET_SOURCE, _abi.VB2_SET_RELATED
    RELATIONS = ("DUP", "PO", "FS", "D2")

    def __init__(self, num_marker, capacity, device=-1, planes=_abi.VB2_SET_SOURCE):
        self._lib = _abi.lib()
        h = C.c_void_p()
        _abi.check(self._lib.vb2_source_set_create_ex(int(num_marker), int(capacity), int(device), int(planes), C.byref(h)),
                   "vb2_source_set_create_ex")
        self._h = h
        self.planes = int(planes)

    @property
    def count(self):
        """Slots taken so far, as the library counts them (vb2_source_set_size)."""
        n = C.c_int32(0)
        _abi.check(self._lib.vb2_source_set_size(self._h, C.byref(n)), "vb2_source_set_size")
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_source_set_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, ctx, estimate, **model_kw):
        """Adds the sample of a LikelihoodContext at an estimate of its optimize(**model_kw); returns its index."""
        m, keep = _model(known_af=ctx.data.known_af is not None, **model_kw)
        est = _estimate_struct(estimate, ctx.num_pc)
        idx = C.c_int32(-1)
        _abi.check(self._lib.vb2_source_set_add(self._h, ctx._h, C.byref(m), C.byref(est), C.byref(idx)),
                   "vb2_source_set_add")
        return idx.value

    def scores(self):
        """(score [n, n] float64, NaN on the diagonal; shared [n, n] int32): row = target, column = candidate."""
        n = self.count
        score, shared = np.zeros((n, n)), np.zeros((n, n), dtype=np.int32)
        _abi.check(self._lib.vb2_source_set_scores(self._h, _p(score), _p(shared)), "vb2_source_set_scores")
        return score, shared

    def relations(self):
        """(llr [n, n, 4] float64 in the order of RELATIONS, NaN on the diagonal; shared [n, n] int32): row = target,
        column = partner (vb2_source_set_relations; a set with the RELATED planes)."""
        n = self.count
        llr, shared = np.zeros((n, n, _abi.VB2_NUM_RELATION)), np.zeros((n, n), dtype=np.int32)
        _abi.check(self._lib.vb2_source_set_relations(self._h, _p(llr), _p(shared)), "vb2_source_set_relations")
        return llr, shared


class CohortBatch:
    """vb2_batch: several LikelihoodContexts (one device, same --NumPC) evaluated and
    optimised in lock-step, one kernel launch per step for the whole cohort."""
    SLOTS = 8

    def __init__(self, contexts):
        self._lib = _abi.lib()
        self.contexts = list(contexts)
        self.num_pc = self.contexts[0].num_pc
        n = len(self.contexts)
        arr = (C.c_void_p * n)(*[c._h for c in self.contexts])
        h = C.c_void_p()
        _abi.check(self._lib.vb2_batch_create(arr, n, C.byref(h)), "vb2_batch_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def eval(self, num_point, pc1, pc2, alpha):
        """num_point: [S] ints (0..8); pc1/pc2: [S,8,k]; alpha: [S,8] -> llk [S,8]."""
        S, k = len(self.contexts), self.num_pc
        npt = np.ascontiguousarray(num_point, dtype=np.int32)
        pc1 = np.ascontiguousarray(pc1, dtype=np.float64).reshape(S, self.SLOTS, k)
        pc2 = np.ascontiguousarray(pc2, dtype=np.float64).reshape(S, self.SLOTS, k)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(S, self.SLOTS)
        out = np.zeros((S, self.SLOTS))
        _abi.check(self._lib.vb2_batch_eval(self._h, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(out)),
                   "vb2_batch_eval")
        return out

    def prepared_eval(self, num_point, pc1, pc2, alpha):
        """The same call with the argument marshalling done once: returns (step, out) where step() makes one
        vb2_batch_eval call on the captured arrays (bench.py times steps, not numpy conversions)."""
        S, k = len(self.contexts), self.num_pc
        npt = np.ascontiguousarray(num_point, dtype=np.int32)
        pc1 = np.ascontiguousarray(pc1, dtype=np.float64).reshape(S, self.SLOTS, k)
        pc2 = np.ascontiguousarray(pc2, dtype=np.float64).reshape(S, self.SLOTS, k)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(S, self.SLOTS)
        out = np.zeros((S, self.SLOTS))
        fn, h, a = self._lib.vb2_batch_eval, self._h, (_p(npt), _p(pc1), _p(pc2), _p(alpha), _p(out))
        keep = (npt, pc1, pc2, alpha)

        def step(_keep=keep):
            rc = fn(h, *a)
            if rc:
                _abi.check(rc, "vb2_batch_eval")
        return step, out

    def optimize(self, models=None, **model_kw):
        """Every sample's OptimizeLLK in lock-step (vb2_batch_optimize_llk).  model_kw: one model for all samples;
        models: a list of one keyword dict per sample instead (the library refuses any other length).  A sample with
        a known-AF column is searched over alpha alone whatever its model says (estimator.h: apply_model)."""
        S = len(self.contexts)
        if models is None:
            m, keep = _model(**model_kw)
            arr, n = C.byref(m), 1
        else:
            built = [_model(**dict(model_kw, **kw)) for kw in models]
            keep = [fpc for _, fpc in built]              # (the fix_pc arrays the structs point into)
            n = len(built)
            arr = (_abi.Model * max(1, n))(*[m for m, _ in built])
        est = (_abi.Estimate * S)()
        _abi.check(self._lib.vb2_batch_optimize_llk(self._h, arr, n, est),
                   "vb2_batch_optimize_llk")
        return [_estimate_dict(est[s], self.num_pc) for s in range(S)]


    def derivatives(self, num_point, pc1, pc2, alpha):
        """LLK, gradient and Hessian of every sample at its own points in one launch pair per step (vb2_batch_derivs):
        num_point [S] ints >= 0; pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point), the samples' rows one after the
        other.  Returns (llk [P], grad [P, 2k+1], hess [P, 2k+1, 2k+1]): every row is the bits of
        LikelihoodContext.derivatives on that sample alone."""
        S, k = len(self.contexts), self.num_pc
        npt = np.ascontiguousarray(num_point, dtype=np.int32).reshape(S)
        P = int(npt.sum())
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(P, k))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(P, k))
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(P))
        n = 2 * k + 1
        llk, grad, hess = np.zeros(P), np.zeros((P, n)), np.zeros((P, n, n))
        _abi.check(self._lib.vb2_batch_derivs(self._h, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(llk), _p(grad), _p(hess)),
                   "vb2_batch_derivs")
        return llk, grad, hess

    def intervals(self, estimates, **model_kw):
        """LikelihoodContext.interval for every sample at estimates[s] (of optimize(**model_kw)), advancing in lock-step
        (vb2_batch_interval): one dict per sample, with its own "status"; every number is what the sample's context gives
        alone, bit for bit.  self.num_interval_step: the batched derivative steps the call took."""
        S = len(self.contexts)
        built = [_model(known_af=c.data.known_af is not None, **model_kw) for c in self.contexts]
        keep = [fpc for _, fpc in built]                  # (the fix_pc arrays the structs point into)
        models = (_abi.Model * S)(*[m for m, _ in built])
        est = (_abi.Estimate * S)(*[_estimate_struct(e, self.num_pc) for e in estimates])
        ci = (_abi.Interval * S)()
        status = (C.c_int32 * S)()
        steps = C.c_int64(0)
        _abi.check(self._lib.vb2_batch_interval(self._h, models, S, est, ci, status, C.byref(steps)), "vb2_batch_interval")
        del keep
        self.num_interval_step = int(steps.value)
        return [dict(_interval_dict(ci[s]), status=int(status[s])) for s in range(S)]


def _step_points(n, npt, p1, p2, a, k):
    """What a lock-step driver hands a step's callback, as arrays of the callback's own: (num_point [n] int32, pc1 [P, k],
    pc2 [P, k], alpha [P]) and P = sum(num_point)."""
    num_point = np.ctypeslib.as_array(npt, (n,)).copy()
    P = int(num_point.sum())
    return (num_point, np.ctypeslib.as_array(p1, (P, k)).copy(), np.ctypeslib.as_array(p2, (P, k)).copy(),
            np.ctypeslib.as_array(a, (P,)).copy()), P


def intervals_with_evaluator(evaluate, num_pc, estimates, known_af=None, **model_kw):
    """The lock-step interval driver over a Python evaluator (vb2_intervals_lockstep): no device.
    evaluate(num_point [S] int32, pc1 [P, k], pc2 [P, k], alpha [P]) -> (llk [P], grad [P, 2k+1], hess [P, 2k+1, 2k+1]),
    P = sum(num_point), called once per step -- on the calling thread's own stack -- with one point of every sample whose
    interval is still running.  known_af: None or one flag per sample.  Returns (intervals, num_step): one dict per sample
    (with "status") and the calls made."""
    L = _abi.lib()
    k, S = int(num_pc), len(estimates)
    n = 2 * k + 1
    err = []

    def cb(_user, ns, npt, p1, p2, a, llk, grad, hess):
        try:
            points, P = _step_points(ns, npt, p1, p2, a, k)
            res = evaluate(*points)
            np.ctypeslib.as_array(llk, (P,))[:] = np.asarray(res[0], dtype=np.float64).reshape(P)
            np.ctypeslib.as_array(grad, (P, n))[:] = np.asarray(res[1], dtype=np.float64).reshape(P, n)
            np.ctypeslib.as_array(hess, (P, n, n))[:] = np.asarray(res[2], dtype=np.float64).reshape(P, n, n)
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fn = _abi.BATCH_DERIVS_FN(cb)
    flags = [bool(f) for f in known_af] if known_af is not None else [False] * S
    built = [_model(known_af=f, **model_kw) for f in flags]
    keep = [fpc for _, fpc in built]
    models = (_abi.Model * S)(*[m for m, _ in built])
    kaf = (C.c_int32 * S)(*[int(f) for f in flags])
    est = (_abi.Estimate * S)(*[_estimate_struct(e, k) for e in estimates])
    ci = (_abi.Interval * S)()
    status = (C.c_int32 * S)()
    steps = C.c_int64(0)
    rc = L.vb2_intervals_lockstep(fn, None, S, k, kaf, models, S, est, ci, status, C.byref(steps))
    del keep
    if err:
        raise err[0]
    _abi.check(rc, "vb2_intervals_lockstep")
    return [dict(_interval_dict(ci[s]), status=int(status[s])) for s in range(S)], int(steps.value)


class _RowSet:
    """What Replicates, Conditioned and Paired share: the life of the handle and one step.  A class says which entries are
    its own (_NAME: vb2_<_NAME>_eval, vb2_<_NAME>_destroy) and which attribute holds its rows' number (_ROWS)."""
    SLOTS = _abi.VB2_BATCH_SLOTS
    _NAME = _ROWS = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, "vb2_%s_destroy" % self._NAME)(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _eval(self, num_point, pc1, pc2, alpha):
        k, where = self.num_pc, "vb2_%s_eval" % self._NAME
        npt = np.ascontiguousarray(num_point, dtype=np.int32).reshape(getattr(self, self._ROWS))
        P = int(npt.sum())
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(P, k))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(P, k))
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(P))
        out = np.zeros(P)
        _abi.check(getattr(self._lib, where)(self._h, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(out)), where)
        return out


def _optimize_sets(symbol, sets, fixed, **model_kw):
    """vb2_conditioned_optimize_llk / vb2_paired_optimize_llk (`symbol`) over `sets`, their held PCs fixed [num_set, k]:
    per set a list of dicts, one per hypothesis (with "status")."""
    k = sets[0].num_pc
    S = len(sets)
    fixed = np.ascontiguousarray(np.asarray(fixed, dtype=np.float64).reshape(S, k))
    m, keep = _model(**model_kw)
    H = sum(c.num_hyp for c in sets)
    handles = (C.c_void_p * S)(*[c._h for c in sets])
    est = (_abi.Estimate * H)()
    status = (C.c_int32 * H)()
    _abi.check(getattr(_abi.lib(), symbol)(handles, S, C.byref(m), _p(fixed), est, status), symbol)
    del keep
    out, at = [], 0
    for c in sets:
        out.append([dict(_estimate_dict(est[at + h], k), status=int(status[at + h])) for h in range(c.num_hyp)])
        at += c.num_hyp
    return out


def _rows_with_evaluator(fn_type, symbol, evaluate, n, k, fixed, known_af, **model_kw):
    """A lock-step driver over a Python evaluator (`symbol`: vb2_replicates_lockstep, vb2_conditioned_lockstep,
    vb2_paired_lockstep; its callback type fn_type): n rows, fixed [n, k] the held PCs or None where the driver takes
    none.  One dict per row (with "status")."""
    k, n = int(k), int(n)
    err = []

    def cb(_user, rows, npt, p1, p2, a, out):
        try:
            points, P = _step_points(rows, npt, p1, p2, a, k)
            np.ctypeslib.as_array(out, (P,))[:] = np.asarray(evaluate(*points), dtype=np.float64).reshape(P)
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fn = fn_type(cb)
    if fixed is not None:
        fixed = np.ascontiguousarray(np.asarray(fixed, dtype=np.float64).reshape(n, k))
    held = [] if fixed is None else [_p(fixed)]
    m, keep = _model(known_af=known_af, **model_kw)
    est = (_abi.Estimate * n)()
    status = (C.c_int32 * n)()
    rc = getattr(_abi.lib(), symbol)(fn, None, n, k, C.byref(m), *held, est, status)
    del keep
    if err:
        raise err[0]
    _abi.check(rc, symbol)
    return [dict(_estimate_dict(est[r], k), status=int(status[r])) for r in range(n)]


class Replicates(_RowSet):
    """vb2_replicates: many integer weight vectors ("replicates") over the ONE resident copy of a sample -- the
    log-likelihood under marker weights, LLK_w = sum_i w_i log L_i, evaluated for all of them together and searched in
    lock-step.  weights: [R, M] counts 0..255 in panel order (chromosome_weights, bootstrap_weights, or the caller's)."""
    _NAME, _ROWS = "replicates", "num_rep"

    def __init__(self, ctx: LikelihoodContext, weights):
        self._lib = _abi.lib()
        self.ctx = ctx
        self.num_pc = ctx.num_pc
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights)))
        if w.shape[1] != ctx.data.num_marker:
            raise ValueError("weights must be [replicates, %d markers]" % ctx.data.num_marker)
        if w.min() < 0 or w.max() > 255:
            raise ValueError("weights are counts 0..255")
        w = np.ascontiguousarray(w, dtype=np.uint8)
        self.num_rep = int(w.shape[0])
        h = C.c_void_p()
        _abi.check(self._lib.vb2_replicates_create(ctx._h, self.num_rep, _p(w), C.byref(h)), "vb2_replicates_create")
        self._h = h

    def info(self):
        i = _abi.ReplicatesInfo()
        counted = np.zeros(self.num_rep, dtype=np.int64)
        _abi.check(self._lib.vb2_replicates_info_get(self._h, C.byref(i), _p(counted)), "vb2_replicates_info_get")
        return dict(num_rep=i.num_rep, num_marker=i.num_marker, device_bytes=int(i.device_bytes), num_step=int(i.num_step),
                    num_launch=int(i.num_launch), counted=counted)

    def eval(self, num_point, pc1, pc2, alpha):
        """One step (vb2_replicates_eval): num_point [R] ints 0..8; pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point),
        the replicates' rows one after the other.  Returns llk [P]."""
        return self._eval(num_point, pc1, pc2, alpha)

    def optimize(self, **model_kw):
        """OptimizeLLK of every replicate in lock-step (vb2_replicates_optimize_llk): one dict per replicate with its own
        "status" (VB2_ERR_INVALID: the replicate's weights select no counted marker)."""
        m, keep = _model(known_af=self.ctx.data.known_af is not None, **model_kw)
        est = (_abi.Estimate * self.num_rep)()
        status = (C.c_int32 * self.num_rep)()
        _abi.check(self._lib.vb2_replicates_optimize_llk(self._h, C.byref(m), est, status), "vb2_replicates_optimize_llk")
        del keep
        return [dict(_estimate_dict(est[r], self.num_pc), status=int(status[r])) for r in range(self.num_rep)]


def replicates_with_evaluator(evaluate, num_rep, num_pc, known_af=False, **model_kw):
    """The replicates' lock-step driver over a Python evaluator (vb2_replicates_lockstep): no device.
    evaluate(num_point [R] int32, pc1 [P, k], pc2 [P, k], alpha [P]) -> llk [P], P = sum(num_point), called once per step
    with the points of every replicate still searching.  Returns one dict per replicate (with "status")."""
    return _rows_with_evaluator(_abi.REPLICATES_EVAL_FN, "vb2_replicates_lockstep", evaluate, num_rep, num_pc, None, known_af,
                                **model_kw)


class Conditioned(_RowSet):
    """vb2_conditioned: the likelihood of the ONE resident sample given a hypothesised contaminant -- per hypothesis one
    genotype triple per panel marker (float32, panel order) in place of the Hardy-Weinberg prior of the alpha-fraction
    component; an all-zero triple falls back to that prior.  prior: [H, M, 3]; or source_set= and candidates= (indices
    into a SourceSet on the context's device): hypothesis h is the genotype posterior of that sample, copied on the device."""
    _NAME, _ROWS = "conditioned", "num_hyp"

    def __init__(self, ctx: LikelihoodContext, prior=None, source_set=None, candidates=None):
        self._lib = _abi.lib()
        self.ctx = ctx
        self.num_pc = ctx.num_pc
        h = C.c_void_p()
        if source_set is not None:
            cand = np.ascontiguousarray(np.atleast_1d(np.asarray(candidates)), dtype=np.int32)
            self.num_hyp = int(cand.shape[0])
            _abi.check(self._lib.vb2_conditioned_create_from_set(ctx._h, source_set._h, self.num_hyp, _p(cand), C.byref(h)),
                       "vb2_conditioned_create_from_set")
        else:
            pr = np.asarray(prior)
            if pr.ndim == 2:
                pr = pr[None]
            if pr.ndim != 3 or pr.shape[1:] != (ctx.data.num_marker, 3):
                raise ValueError("prior must be [hypotheses, %d markers, 3]" % ctx.data.num_marker)
            pr = np.ascontiguousarray(pr, dtype=np.float32)
            self.num_hyp = int(pr.shape[0])
            _abi.check(self._lib.vb2_conditioned_create(ctx._h, self.num_hyp, _p(pr), C.byref(h)), "vb2_conditioned_create")
        self._h = h

    def info(self):
        i = _abi.ConditionedInfo()
        _abi.check(self._lib.vb2_conditioned_info_get(self._h, C.byref(i)), "vb2_conditioned_info_get")
        return dict(num_hyp=i.num_hyp, num_marker=i.num_marker, device_bytes=int(i.device_bytes), num_step=int(i.num_step),
                    num_launch=int(i.num_launch))

    def eval(self, num_point, pc1, pc2, alpha):
        """One step (vb2_conditioned_eval): num_point [H] ints 0..8; pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point),
        the hypotheses' rows one after the other.  Returns llk [P]."""
        return self._eval(num_point, pc1, pc2, alpha)

    def optimize(self, pc1_fixed, **model_kw):
        """The refit of every hypothesis in lock-step (Conditioned.optimize_sets on this set alone)."""
        return Conditioned.optimize_sets([self], [pc1_fixed], **model_kw)[0]

    @staticmethod
    def optimize_sets(sets, pc1_fixed, **model_kw):
        """vb2_conditioned_optimize_llk: the refits of every hypothesis of every set in ONE lock-step gang -- alpha and the
        intended sample's PCs (alpha alone with fix_pc= or known allele frequencies), the contaminant's PCs held at
        pc1_fixed[s] ([num_set, k]).  Returns per set a list of dicts (alpha, pc2 -- also in pc --, llk1, llk0, "status")."""
        return _optimize_sets("vb2_conditioned_optimize_llk", sets, pc1_fixed, **model_kw)


def conditioned_with_evaluator(evaluate, num_hyp, num_pc, pc1_fixed, known_af=False, **model_kw):
    """The refits' lock-step driver over a Python evaluator (vb2_conditioned_lockstep): no device.
    evaluate(num_point [H] int32, pc1 [P, k], pc2 [P, k], alpha [P]) -> llk [P], P = sum(num_point), called once per step
    with the points of every hypothesis still searching; the pc1 rows are pc1_fixed [H, k] at every call.  Returns one dict
    per hypothesis (with "status")."""
    return _rows_with_evaluator(_abi.CONDITIONED_EVAL_FN, "vb2_conditioned_lockstep", evaluate, num_hyp, num_pc, pc1_fixed,
                                known_af, **model_kw)


def _refbias_fit_dict(f, k):
    n = int(f.num_pair)
    return dict(beta=f.beta, beta_se=f.beta_se, at_bound=bool(f.at_bound), alpha_bias=f.alpha_bias,
                freemix_bias=min(f.alpha_bias, 1 - f.alpha_bias), pc=np.array(f.pc[:k]), pc2=np.array(f.pc2[:k]),
                llk1_bias=f.llk1_bias, llk1_at_half=f.llk1_at_half, alpha_at_half=f.alpha_at_half, lrt=f.lrt,
                num_round=int(f.num_round), num_refit=int(f.num_refit), num_step=int(f.num_step), status=int(f.status),
                pairs=[(f.pair_beta[i], f.pair_llk1[i]) for i in range(n)])


class RefBias(_RowSet):
    """vb2_refbias: the likelihood of the ONE resident sample under a reference bias -- beta = P(an error-free read of a
    heterozygous genotype shows REF) in place of the model's 0.5 --, one beta in [0.25, 0.75] per row: evaluated for all
    rows together and refitted in lock-step.  RefBias.fit(ctx) is the whole estimate of beta (vb2_refbias_fit_ctx).  Every
    llk1 of a fit is a log-likelihood (.selfSM's FREELK1); the estimates of optimize() are vb2_estimate's, as everywhere."""
    _NAME, _ROWS = "refbias", "num_row"

    def __init__(self, ctx: LikelihoodContext, beta):
        self._lib = _abi.lib()
        self.ctx = ctx
        self.num_pc = ctx.num_pc
        b = np.ascontiguousarray(np.atleast_1d(np.asarray(beta, dtype=np.float64)))
        if b.ndim != 1:
            raise ValueError("beta must be [rows]")
        self.num_row = int(b.shape[0])
        h = C.c_void_p()
        _abi.check(self._lib.vb2_refbias_create(ctx._h, self.num_row, _p(b), C.byref(h)), "vb2_refbias_create")
        self._h = h

    def info(self):
        i = _abi.RefBiasInfo()
        _abi.check(self._lib.vb2_refbias_info_get(self._h, C.byref(i)), "vb2_refbias_info_get")
        return dict(num_row=i.num_row, num_marker=i.num_marker, device_bytes=int(i.device_bytes), num_step=int(i.num_step),
                    num_launch=int(i.num_launch))

    def eval(self, num_point, pc1, pc2, alpha):
        """One step (vb2_refbias_eval): num_point [R] ints 0..8; pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point), the
        rows' points one after the other.  Returns llk [P]."""
        return self._eval(num_point, pc1, pc2, alpha)

    def optimize(self, **model_kw):
        """The profile refit of every row in lock-step (vb2_refbias_optimize_llk): one dict per row (with "status")."""
        m, keep = _model(known_af=self.ctx.data.known_af is not None, **model_kw)
        est = (_abi.Estimate * self.num_row)()
        status = (C.c_int32 * self.num_row)()
        _abi.check(self._lib.vb2_refbias_optimize_llk(self._h, C.byref(m), est, status), "vb2_refbias_optimize_llk")
        del keep
        return [dict(_estimate_dict(est[r], self.num_pc), status=int(status[r])) for r in range(self.num_row)]

    @staticmethod
    def fit(ctx: LikelihoodContext, **model_kw):
        """vb2_refbias_fit_ctx: beta, beta_se, at_bound, alpha_bias (freemix_bias: folded), pc, pc2, llk1_bias, llk1_at_half,
        alpha_at_half, lrt, the counters and `pairs`, the 28 (beta, llk1) in the order evaluated."""
        m, keep = _model(known_af=ctx.data.known_af is not None, **model_kw)
        f = _abi.RefBiasFit()
        _abi.check(_abi.lib().vb2_refbias_fit_ctx(ctx._h, C.byref(m), C.byref(f)), "vb2_refbias_fit_ctx")
        del keep
        return _refbias_fit_dict(f, ctx.num_pc)


def refbias_with_evaluator(evaluate, num_pc, known_af=False, **model_kw):
    """The estimate of beta over a Python evaluator (vb2_refbias_lockstep): no device.
    evaluate(beta [R], num_point [R] int32, pc1 [P, k], pc2 [P, k], alpha [P]) -> llk [P], P = sum(num_point), called once
    per step with the rows of the lock-step call in hand and the points of every row still searching.  Returns the dict of
    RefBias.fit; a search that fails raises with its status in the message's code."""
    k = int(num_pc)
    err = []

    def cb(_user, rows, npt, beta, p1, p2, a, out):
        try:
            points, P = _step_points(rows, npt, p1, p2, a, k)
            b = np.ctypeslib.as_array(beta, (rows,)).copy()
            np.ctypeslib.as_array(out, (P,))[:] = np.asarray(evaluate(b, *points), dtype=np.float64).reshape(P)
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fn = _abi.REFBIAS_EVAL_FN(cb)
    m, keep = _model(known_af=known_af, **model_kw)
    f = _abi.RefBiasFit()
    rc = _abi.lib().vb2_refbias_lockstep(fn, None, k, C.byref(m), int(bool(known_af)), C.byref(f))
    del keep
    if err:
        raise err[0]
    _abi.check(rc, "vb2_refbias_lockstep")
    return _refbias_fit_dict(f, k)


class ErrStat:
    """vb2_errstat: the E-step of the error-rate fit on a device copy of the raw sample -- per clamped quality the reads of
    the counted markers and the expected number of error reads among them, at one point under one error table."""

    def __init__(self, data: PileupData, device=-1, stream=None):
        self._lib = _abi.lib()
        self.data = data
        self.num_pc = data.num_pc
        inp = data.as_input()
        opt = _abi.Options(int(device), 0, C.c_void_p(stream) if stream else None)
        h = C.c_void_p()
        _abi.check(self._lib.vb2_errstat_create(C.byref(inp), C.byref(opt), C.byref(h)), "vb2_errstat_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_errstat_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        i = _abi.ErrStatInfo()
        _abi.check(self._lib.vb2_errstat_info_get(self._h, C.byref(i)), "vb2_errstat_info_get")
        return dict(num_marker=i.num_marker, num_pc=i.num_pc, num_read=int(i.num_read), device_bytes=int(i.device_bytes),
                    num_launch=int(i.num_launch))

    def eval(self, err_table, pc1, pc2, alpha):
        """vb2_errstat_eval: (n [94] int64, s [94], llk) at (pc1 [k], pc2 [k], alpha) under err_table [94]."""
        e = _err_table(err_table)
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(-1))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(-1))
        assert pc1.shape == (self.num_pc,) and pc2.shape == (self.num_pc,)
        n, s, llk = np.zeros(_abi.VB2_ERR_NUM_QUAL, dtype=np.int64), np.zeros(_abi.VB2_ERR_NUM_QUAL), C.c_double(0.0)
        _abi.check(self._lib.vb2_errstat_eval(self._h, _p(e), _p(pc1), _p(pc2), float(alpha), _p(n), _p(s), C.byref(llk)),
                   "vb2_errstat_eval")
        return n, s, llk.value


class ErrStatBatch:
    """vb2_errstat_batch: the E-steps of up to 64 samples in one launch pair, every sample at its own point under its own
    error table.  `samples` is a list of PileupData; None stands for a sample that holds nothing.  Samples whose ud and
    means (or known_af) are the same arrays share one device copy.  What a sample gets is ErrStat.eval's bits."""

    def __init__(self, samples, device=-1, stream=None):
        self._lib = _abi.lib()
        self.samples = list(samples)
        S = self.num_sample = len(self.samples)
        self._inputs = [None if d is None else d.as_input() for d in self.samples]
        ptrs = (C.POINTER(_abi.Input) * max(S, 1))(*[C.POINTER(_abi.Input)() if i is None else C.pointer(i) for i in self._inputs])
        opt = _abi.Options(int(device), 0, C.c_void_p(stream) if stream else None)
        h = C.c_void_p()
        _abi.check(self._lib.vb2_errstat_batch_create(ptrs, S, C.byref(opt), C.byref(h)), "vb2_errstat_batch_create")
        self._h = h
        self.num_pc = self.info()["num_pc"]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_errstat_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        i = _abi.ErrStatBatchInfo()
        _abi.check(self._lib.vb2_errstat_batch_info_get(self._h, C.byref(i)), "vb2_errstat_batch_info_get")
        return {n: int(getattr(i, n)) for n, _ in _abi.ErrStatBatchInfo._fields_}

    def eval(self, err_tables, pc1, pc2, alpha, live=None):
        """vb2_errstat_batch_eval: (n [S, 94] int64, s [S, 94], llk [S]).  err_tables [S, 94], or [94] for one table shared
        by all; pc1 / pc2: per sample a vector of its own num_pc entries (a list, or an array [S, num_pc]; None with known
        allele frequencies throughout); alpha [S]; live [S] or None (all)."""
        S, Q, k = self.num_sample, _abi.VB2_ERR_NUM_QUAL, self.num_pc
        e = np.asarray(err_tables, dtype=np.float64)
        e = np.ascontiguousarray(np.broadcast_to(e, (S, Q)) if e.ndim == 1 else e.reshape(S, Q))

        def rows(pc):
            if pc is None:
                return None
            out = np.zeros((S, k))
            for i in range(S):
                v = np.asarray(pc[i], dtype=np.float64).reshape(-1)
                out[i, :min(k, v.shape[0])] = v[:k]
            return out
        p1, p2 = rows(pc1), rows(pc2)
        a = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(S))
        lv = None if live is None else np.ascontiguousarray(np.asarray(live).reshape(S), dtype=np.int32)
        n, s, llk = np.zeros((S, Q), dtype=np.int64), np.zeros((S, Q)), np.zeros(S)
        _abi.check(self._lib.vb2_errstat_batch_eval(self._h, _p(lv), _p(e), _p(p1), _p(p2), _p(a), _p(n), _p(s), _p(llk)),
                   "vb2_errstat_batch_eval")
        return n, s, llk


def _errfit_opts(prior_reads=0.0, tol=0.0, max_iter=0):
    return _abi.ErrFitOpts(float(prior_reads), float(tol), int(max_iter), 0)


def _errfit_dict(f, k):
    t = int(f.num_iter)
    return dict(err=np.array(f.err[:]), n=np.array(f.n[:], dtype=np.int64), s=np.array(f.s[:]),
                estimate=_estimate_dict(f.est, k), alpha_fit=f.est.alpha, freemix_fit=min(f.est.alpha, 1 - f.est.alpha),
                llk_fit=f.llk_fit, llk_nominal=f.llk_nominal, alpha_nominal=f.alpha_nominal, lrt=f.lrt,
                num_bin=int(f.num_bin), num_iter=t, converged=bool(f.converged), num_step=int(f.num_step), status=int(f.status),
                iter_llk=np.array(f.iter_llk[:t]), iter_change=np.array(f.iter_change[:t]), iter_alpha=np.array(f.iter_alpha[:t]),
                iter_err=np.array([list(f.iter_err[i]) for i in range(t)], dtype=np.float32).reshape(t, _abi.VB2_ERR_NUM_QUAL))


def errfit(data: PileupData, nominal, device=-1, prior_reads=0.0, tol=0.0, max_iter=0, **model_kw):
    """vb2_errfit_input: the error rates per quality fitted jointly with the model's parameters on the device, starting
    from `nominal`, the estimate of optimize(**model_kw) on a context of `data`.  Returns err, n, s [94], estimate (the final
    search), llk_fit, llk_nominal, lrt, num_bin, num_iter, converged and the per-iteration iter_llk, iter_change, iter_alpha,
    iter_err."""
    m, keep = _model(known_af=data.known_af is not None, **model_kw)
    inp = data.as_input()
    opt = _abi.Options(int(device), 0, None)
    est = _estimate_struct(nominal, data.num_pc)
    o = _errfit_opts(prior_reads, tol, max_iter)
    f = _abi.ErrFit()
    _abi.check(_abi.lib().vb2_errfit_input(C.byref(inp), C.byref(opt), C.byref(m), C.byref(est), C.byref(o), C.byref(f)),
               "vb2_errfit_input")
    del keep
    return _errfit_dict(f, data.num_pc)


def errfit_with_evaluator(evaluate, stats, num_pc, nominal, known_af=False, prior_reads=0.0, tol=0.0, max_iter=0, **model_kw):
    """The same fit over two Python callbacks (vb2_errfit_lockstep): no device.
    evaluate(err [94], pc1 [B, k], pc2 [B, k], alpha [B]) -> llk [B] answers the searches;
    stats(err [94], pc1 [k], pc2 [k], alpha) -> (n [94], s [94]) is the E-step.  Returns the dict of errfit."""
    k = int(num_pc)
    Q = _abi.VB2_ERR_NUM_QUAL
    err = []

    def cb_eval(_user, e, n, p1, p2, a, out):
        try:
            table = np.ctypeslib.as_array(e, (Q,)).copy()
            pc1 = np.ctypeslib.as_array(p1, (n, k)).copy()
            pc2 = np.ctypeslib.as_array(p2, (n, k)).copy()
            al = np.ctypeslib.as_array(a, (n,)).copy()
            np.ctypeslib.as_array(out, (n,))[:] = np.asarray(evaluate(table, pc1, pc2, al), dtype=np.float64).reshape(n)
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID

    def cb_stats(_user, e, p1, p2, a, n_out, s_out):
        try:
            table = np.ctypeslib.as_array(e, (Q,)).copy()
            pc1 = np.ctypeslib.as_array(p1, (k,)).copy()
            pc2 = np.ctypeslib.as_array(p2, (k,)).copy()
            n, s = stats(table, pc1, pc2, float(a))
            np.ctypeslib.as_array(n_out, (Q,))[:] = np.asarray(n, dtype=np.int64).reshape(Q)
            np.ctypeslib.as_array(s_out, (Q,))[:] = np.asarray(s, dtype=np.float64).reshape(Q)
            return 0
        except Exception as exc:
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fns = _abi.ErrFitFns(_abi.ERRFIT_EVAL_FN(cb_eval), _abi.ERRFIT_STATS_FN(cb_stats))
    m, keep = _model(known_af=known_af, **model_kw)
    est = _estimate_struct(nominal, k)
    o = _errfit_opts(prior_reads, tol, max_iter)
    f = _abi.ErrFit()
    rc = _abi.lib().vb2_errfit_lockstep(C.byref(fns), None, k, C.byref(m), int(bool(known_af)), C.byref(est), C.byref(o),
                                        C.byref(f))
    del keep
    if err:
        raise err[0]
    _abi.check(rc, "vb2_errfit_lockstep")
    return _errfit_dict(f, k)


def _errfit_pool_dict(p):
    t = int(p.num_iter) if p.pooled else 0
    out = {n: int(getattr(p, n)) for n in ("num_step", "device_bytes", "num_bin", "num_iter", "num_sample", "num_entered",
                                           "num_fitted", "num_estep")}
    out.update(err=np.array(p.err[:]), n=np.array(p.n[:], dtype=np.int64), s=np.array(p.s[:]), lrt_sum=p.lrt_sum,
               converged=bool(p.converged), pooled=bool(p.pooled), seconds_stats=p.seconds_stats,
               seconds_context=p.seconds_context, seconds_search=p.seconds_search, iter_change=np.array(p.iter_change[:t]),
               iter_err=np.array([list(p.iter_err[i]) for i in range(t)], dtype=np.float32).reshape(t, _abi.VB2_ERR_NUM_QUAL))
    return out


def _cohort_fit_args(nominals, enter_status, k):
    S = len(nominals)
    ests = (_abi.Estimate * S)()
    enter = np.zeros(S, dtype=np.int32) if enter_status is None else np.ascontiguousarray(enter_status, dtype=np.int32).reshape(S)
    for i, nom in enumerate(nominals):
        if nom is not None and enter[i] == 0:
            ests[i] = _estimate_struct(nom, k)
        elif enter[i] == 0:
            raise ValueError("sample %d enters the fit and has no nominal estimate" % i)
    return ests, enter, (_abi.ErrFit * S)(), _abi.ErrFitPool()


def errfit_cohort(samples, nominals, pooled=False, enter_status=None, device=-1, prior_reads=0.0, tol=0.0, max_iter=0, **model_kw):
    """vb2_errfit_cohort_inputs: the error-rate fits of up to 64 samples in lock-step on the device -- every sample on its own
    table, or (pooled=True) all of them on one.  samples: PileupData of one num_pc (None where enter_status is non-zero);
    nominals: each sample's own estimate; enter_status [S]: non-zero for a sample whose own run failed -- it never enters.
    Returns (fits, pool): per sample the dict of errfit (its "status" the code it left with), and the pooled summary."""
    S = len(samples)
    held = [d for i, d in enumerate(samples) if d is not None and (enter_status is None or enter_status[i] == 0)]
    k = held[0].num_pc if held else 1
    m, keep = _model(known_af=bool(held) and held[0].known_af is not None, **model_kw)
    inputs = [None if d is None else d.as_input() for d in samples]
    ptrs = (C.POINTER(_abi.Input) * max(S, 1))(*[C.POINTER(_abi.Input)() if i is None else C.pointer(i) for i in inputs])
    ests, enter, fits, pool = _cohort_fit_args(nominals, enter_status, k)
    opt = _abi.Options(int(device), 0, None)
    o = _errfit_opts(prior_reads, tol, max_iter)
    _abi.check(_abi.lib().vb2_errfit_cohort_inputs(ptrs, S, C.byref(opt), C.byref(m), C.addressof(ests), _p(enter), C.byref(o),
                                                   int(bool(pooled)), C.addressof(fits), C.byref(pool)),
               "vb2_errfit_cohort_inputs")
    del keep
    return [_errfit_dict(f, k) for f in fits], _errfit_pool_dict(pool)


class SearchFailed(Exception):
    """Raised by the evaluate callback of errfit_cohort_with_evaluator: the search of that sample fails with `code`."""

    def __init__(self, code):
        super().__init__("search failed (%d)" % code)
        self.code = int(code)


def errfit_cohort_with_evaluator(evaluate, stats, num_pc, nominals, pooled=False, enter_status=None, known_af=False,
                                 prior_reads=0.0, tol=0.0, max_iter=0, **model_kw):
    """The same fit over two Python callbacks (vb2_errfit_cohort_lockstep): no device.
    evaluate(sample, err [94], pc1 [B, k], pc2 [B, k], alpha [B]) -> llk [B] answers the searches of `sample`;
    stats(live [S], err [S, 94], pc1 [S, k], pc2 [S, k], alpha [S]) -> (n [S, 94], s [S, 94]) is the batched E-step (the rows
    of samples that are not live are ignored).  An evaluate that raises SearchFailed(code) fails that sample's search with
    the code: the sample leaves, the others go on.  Returns (fits, pool) as errfit_cohort."""
    k, S, Q = int(num_pc), len(nominals), _abi.VB2_ERR_NUM_QUAL
    err = []

    def cb_eval(_user, sample, e, n, p1, p2, a, out):
        try:
            table = np.ctypeslib.as_array(e, (Q,)).copy()
            pc1 = np.ctypeslib.as_array(p1, (n, k)).copy()
            pc2 = np.ctypeslib.as_array(p2, (n, k)).copy()
            al = np.ctypeslib.as_array(a, (n,)).copy()
            np.ctypeslib.as_array(out, (n,))[:] = np.asarray(evaluate(int(sample), table, pc1, pc2, al), dtype=np.float64).reshape(n)
            return 0
        except SearchFailed as exc:
            return exc.code
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID

    def cb_stats(_user, num, live, e, p1, p2, a, n_out, s_out):
        try:
            lv = np.ctypeslib.as_array(live, (num,)).copy()
            n, s = stats(lv, np.ctypeslib.as_array(e, (num, Q)).copy(), np.ctypeslib.as_array(p1, (num, k)).copy(),
                         np.ctypeslib.as_array(p2, (num, k)).copy(), np.ctypeslib.as_array(a, (num,)).copy())
            np.ctypeslib.as_array(n_out, (num, Q))[:] = np.asarray(n, dtype=np.int64).reshape(num, Q)
            np.ctypeslib.as_array(s_out, (num, Q))[:] = np.asarray(s, dtype=np.float64).reshape(num, Q)
            return 0
        except Exception as exc:
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fns = _abi.ErrFitCohortFns(_abi.ERRFIT_COHORT_EVAL_FN(cb_eval), _abi.ERRFIT_COHORT_STATS_FN(cb_stats))
    m, keep = _model(known_af=known_af, **model_kw)
    ests, enter, fits, pool = _cohort_fit_args(nominals, enter_status, k)
    o = _errfit_opts(prior_reads, tol, max_iter)
    rc = _abi.lib().vb2_errfit_cohort_lockstep(C.byref(fns), None, S, k, C.byref(m), int(bool(known_af)), C.addressof(ests),
                                               _p(enter), C.byref(o), int(bool(pooled)), C.addressof(fits), C.byref(pool))
    del keep
    if err:
        raise err[0]
    _abi.check(rc, "vb2_errfit_cohort_lockstep")
    return [_errfit_dict(f, k) for f in fits], _errfit_pool_dict(pool)


class Paired(_RowSet):
    """vb2_paired: the likelihood of the ONE resident sample given genotype priors on BOTH components -- per hypothesis two
    float32 triples per panel marker, pi1 for the contaminant and pi2 for the intended sample; an all-zero triple falls back
    to that side's Hardy-Weinberg prior, a negative pi2[0] leaves the marker out.  prior: [H, M, 6] (pi1 | pi2); or
    source_set=, normals= (indices into a SourceSet on the context's device) and hom_min=: hypothesis h is the matched-normal
    rule on that sample's genotype posterior, built on the device."""
    _NAME, _ROWS = "paired", "num_hyp"

    def __init__(self, ctx: LikelihoodContext, prior=None, source_set=None, normals=None, hom_min=0.99):
        self._lib = _abi.lib()
        self.ctx = ctx
        self.num_pc = ctx.num_pc
        h = C.c_void_p()
        if source_set is not None:
            nrm = np.ascontiguousarray(np.atleast_1d(np.asarray(normals)), dtype=np.int32)
            self.num_hyp = int(nrm.shape[0])
            _abi.check(self._lib.vb2_paired_create_from_set(ctx._h, source_set._h, self.num_hyp, _p(nrm), float(hom_min),
                                                            C.byref(h)), "vb2_paired_create_from_set")
        else:
            pr = np.asarray(prior)
            if pr.ndim == 2:
                pr = pr[None]
            if pr.ndim != 3 or pr.shape[1:] != (ctx.data.num_marker, 6):
                raise ValueError("prior must be [hypotheses, %d markers, 6]" % ctx.data.num_marker)
            pr = np.ascontiguousarray(pr, dtype=np.float32)
            self.num_hyp = int(pr.shape[0])
            _abi.check(self._lib.vb2_paired_create(ctx._h, self.num_hyp, _p(pr), C.byref(h)), "vb2_paired_create")
        self._h = h

    def info(self):
        i = _abi.PairedInfo()
        given = np.zeros(self.num_hyp, dtype=np.int64)
        _abi.check(self._lib.vb2_paired_info_get(self._h, C.byref(i), _p(given)), "vb2_paired_info_get")
        return dict(num_hyp=i.num_hyp, num_marker=i.num_marker, device_bytes=int(i.device_bytes), num_step=int(i.num_step),
                    num_launch=int(i.num_launch), given=given)

    def eval(self, num_point, pc1, pc2, alpha):
        """One step (vb2_paired_eval): num_point [H] ints 0..8; pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point),
        the hypotheses' rows one after the other.  Returns llk [P]."""
        return self._eval(num_point, pc1, pc2, alpha)

    def optimize(self, pc2_fixed, **model_kw):
        """The refit of every hypothesis in lock-step (Paired.optimize_sets on this set alone)."""
        return Paired.optimize_sets([self], [pc2_fixed], **model_kw)[0]

    @staticmethod
    def optimize_sets(sets, pc2_fixed, **model_kw):
        """vb2_paired_optimize_llk: the refits of every hypothesis of every set in ONE lock-step gang -- alpha and the
        contaminant's PCs (alpha alone with fix_pc= or known allele frequencies), the intended sample's PCs held at
        pc2_fixed[s] ([num_set, k]).  Returns per set a list of dicts (alpha, pc -- the contaminant's --, llk1, llk0,
        "status")."""
        return _optimize_sets("vb2_paired_optimize_llk", sets, pc2_fixed, **model_kw)


    def derivatives(self, num_point, pc1, pc2, alpha):
        """LLK(. | h), its gradient and Hessian with respect to (pc1[0..k), pc2[0..k), alpha) (vb2_paired_derivs): num_point
        [H] ints >= 0 (any number); pc1 / pc2 [P, k] and alpha [P] with P = sum(num_point), the hypotheses' rows one after the
        other.  Returns (llk [P], grad [P, 2k+1], hess [P, 2k+1, 2k+1]).  Where a side's prior is given its PC entries are
        0; a left-out marker adds nothing; at alpha 0 or 1 the alpha entries are not defined."""
        k = self.num_pc
        npt = np.ascontiguousarray(num_point, dtype=np.int32).reshape(self.num_hyp)
        P = int(npt.sum())
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(P, k))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(P, k))
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(P))
        n = 2 * k + 1
        llk, grad, hess = np.zeros(P), np.zeros((P, n)), np.zeros((P, n, n))
        _abi.check(self._lib.vb2_paired_derivs(self._h, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(llk), _p(grad), _p(hess)),
                   "vb2_paired_derivs")
        return llk, grad, hess

    @staticmethod
    def derivatives_sets(sets, num_point, pc1, pc2, alpha):
        """derivatives for every hypothesis of several sets -- on different contexts of one device -- in one launch pair per
        chunk (vb2_paired_derivs_sets): num_point [sum of num_hyp] in set order.  Every row is the bits of derivatives on
        its own set."""
        k, S = sets[0].num_pc, len(sets)
        npt = np.ascontiguousarray(num_point, dtype=np.int32).reshape(sum(c.num_hyp for c in sets))
        P = int(npt.sum())
        pc1 = np.ascontiguousarray(np.asarray(pc1, dtype=np.float64).reshape(P, k))
        pc2 = np.ascontiguousarray(np.asarray(pc2, dtype=np.float64).reshape(P, k))
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(P))
        n = 2 * k + 1
        llk, grad, hess = np.zeros(P), np.zeros((P, n)), np.zeros((P, n, n))
        handles = (C.c_void_p * S)(*[c._h for c in sets])
        _abi.check(_abi.lib().vb2_paired_derivs_sets(handles, S, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(llk), _p(grad),
                                                     _p(hess)), "vb2_paired_derivs_sets")
        return llk, grad, hess

    def interval(self, estimates, pc2_fixed, **model_kw):
        """The 95 % interval of every hypothesis's refit (Paired.interval_sets on this set alone): one dict per hypothesis."""
        return Paired.interval_sets([self], [estimates], [pc2_fixed], **model_kw)[0][0]

    @staticmethod
    def interval_sets(sets, estimates, pc2_fixed, **model_kw):
        """vb2_paired_interval: the intervals of every hypothesis of every set in ONE lock-step gang, every step one launch
        pair.  estimates: per set the list optimize_sets returned under the same model and pc2_fixed [num_set, k].  Returns
        (per set a list of dicts as LikelihoodContext.interval gives them -- "freemix" is alpha as fitted, unfolded, its
        interval within [0, 1]; the rows after the first are the contaminant's PCs; "status" --, the launch pairs taken)."""
        k, S = sets[0].num_pc, len(sets)
        fixed = np.ascontiguousarray(np.asarray(pc2_fixed, dtype=np.float64).reshape(S, k))
        m, keep = _model(**model_kw)
        H = sum(c.num_hyp for c in sets)
        flat = [e for per_set in estimates for e in per_set]
        if len(flat) != H:
            raise ValueError("one estimate per hypothesis of every set")
        handles = (C.c_void_p * S)(*[c._h for c in sets])
        est = (_abi.Estimate * H)(*[_estimate_struct(e, k) for e in flat])
        ci = (_abi.Interval * H)()
        status = (C.c_int32 * H)()
        steps = C.c_int64(0)
        _abi.check(_abi.lib().vb2_paired_interval(handles, S, C.byref(m), _p(fixed), est, ci, status, C.byref(steps)),
                   "vb2_paired_interval")
        del keep
        out, at = [], 0
        for c in sets:
            out.append([dict(_interval_dict(ci[at + h]), status=int(status[at + h])) for h in range(c.num_hyp)])
            at += c.num_hyp
        return out, int(steps.value)


def paired_intervals_with_evaluator(evaluate, num_pc, estimates, fixed, held="pc2", known_af=None, **model_kw):
    """The paired interval driver over a Python derivative evaluator (vb2_paired_intervals_lockstep): no device.
    evaluate as for intervals_with_evaluator, one slot per hypothesis; the rows it sees on the held side ("pc2", "pc1") are
    fixed [H, k] at every call.  held=None: the anonymous model's intervals, fold included (fixed is not read).  Returns
    (intervals, num_step)."""
    L = _abi.lib()
    k, H = int(num_pc), len(estimates)
    n = 2 * k + 1
    err = []

    def cb(_user, ns, npt, p1, p2, a, llk, grad, hess):
        try:
            points, P = _step_points(ns, npt, p1, p2, a, k)
            res = evaluate(*points)
            np.ctypeslib.as_array(llk, (P,))[:] = np.asarray(res[0], dtype=np.float64).reshape(P)
            np.ctypeslib.as_array(grad, (P, n))[:] = np.asarray(res[1], dtype=np.float64).reshape(P, n)
            np.ctypeslib.as_array(hess, (P, n, n))[:] = np.asarray(res[2], dtype=np.float64).reshape(P, n, n)
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fn = _abi.BATCH_DERIVS_FN(cb)
    code = {None: 0, "pc1": 1, "pc2": 2}[held]
    flags = [bool(f) for f in known_af] if known_af is not None else [False] * H
    m, keep = _model(known_af=False, **model_kw)
    kaf = (C.c_int32 * H)(*[int(f) for f in flags])
    fx = None if code == 0 else np.ascontiguousarray(np.asarray(fixed, dtype=np.float64).reshape(H, k))
    est = (_abi.Estimate * H)(*[_estimate_struct(e, k) for e in estimates])
    ci = (_abi.Interval * H)()
    status = (C.c_int32 * H)()
    steps = C.c_int64(0)
    rc = L.vb2_paired_intervals_lockstep(fn, None, H, k, kaf, C.byref(m), code, None if fx is None else _p(fx), est, ci, status,
                                         C.byref(steps))
    del keep
    if err:
        raise err[0]
    _abi.check(rc, "vb2_paired_intervals_lockstep")
    return [dict(_interval_dict(ci[h]), status=int(status[h])) for h in range(H)], int(steps.value)


def paired_with_evaluator(evaluate, num_hyp, num_pc, pc2_fixed, known_af=False, **model_kw):
    """The paired refits' lock-step driver over a Python evaluator (vb2_paired_lockstep): no device.
    evaluate(num_point [H] int32, pc1 [P, k], pc2 [P, k], alpha [P]) -> llk [P], P = sum(num_point), called once per step
    with the points of every hypothesis still searching; the pc2 rows are pc2_fixed [H, k] at every call.  Returns one dict
    per hypothesis (with "status")."""
    return _rows_with_evaluator(_abi.PAIRED_EVAL_FN, "vb2_paired_lockstep", evaluate, num_hyp, num_pc, pc2_fixed, known_af,
                                **model_kw)


def chromosome_weights(bed_path, num_marker=None):
    """The chromosomes of a panel's .bed as blocks, in order of first appearance (vb2_chromosome_weights): a dict with
    names, block_of [M], block_size (distinct positions per block) and the weight rows only / without [C, M] uint8.
    num_marker: the panel's markers (rows of .UD); None = every row of the .bed."""
    L = _abi.lib()
    if num_marker is None:
        with open(bed_path, "rb") as f:
            num_marker = sum(1 for line in f if line.strip())
    M = int(num_marker)
    nb = C.c_int32(0)
    path = str(bed_path).encode()
    _abi.check(L.vb2_chromosome_weights(path, M, 0, C.byref(nb), None, None, None, None, None), "vb2_chromosome_weights")
    B = nb.value
    block_of, size = np.zeros(M, dtype=np.int32), np.zeros(B, dtype=np.int32)
    names = C.create_string_buffer(B * _abi.VB2_CHROM_NAME_LEN)
    only, without = np.zeros((B, M), dtype=np.uint8), np.zeros((B, M), dtype=np.uint8)
    _abi.check(L.vb2_chromosome_weights(path, M, B, C.byref(nb), _p(block_of), _p(size), C.cast(names, C.c_void_p), _p(only),
                                        _p(without)), "vb2_chromosome_weights")
    n = _abi.VB2_CHROM_NAME_LEN
    return dict(names=[names.raw[j * n:(j + 1) * n].split(b"\0")[0].decode() for j in range(B)], block_of=block_of,
                block_size=size, only=only, without=without)


def bootstrap_weights(num_marker, num_rep, seed):
    """[num_rep, num_marker] uint8 multinomial counts of num_marker uniform draws per replicate (vb2_bootstrap_weights)."""
    out = np.zeros((int(num_rep), int(num_marker)), dtype=np.uint8)
    _abi.check(_abi.lib().vb2_bootstrap_weights(int(num_marker), int(num_rep), int(seed), _p(out)), "vb2_bootstrap_weights")
    return out


def jackknife(m, theta_hat, theta_without):
    """Delete-m_j jackknife (vb2_jackknife): block sizes m, the whole-sample estimate and the estimates with each block left
    out -> (estimate, standard error).  Blocks with m = 0 are skipped."""
    m = np.ascontiguousarray(m, dtype=np.int64)
    tw = np.ascontiguousarray(theta_without, dtype=np.float64)
    assert m.shape == tw.shape and m.ndim == 1
    est, se = C.c_double(0), C.c_double(0)
    _abi.check(_abi.lib().vb2_jackknife(len(m), _p(m), float(theta_hat), _p(tw), C.byref(est), C.byref(se)), "vb2_jackknife")
    return est.value, se.value


class ShardGroup:
    """vb2_shard_group: ONE sample's markers sharded over several GPUs, partial LLKs met in one
    RCCL all-reduce per batch (BASELINE.json configs[3]).

    ShardGroup(data, devices=[0, 1, ...])            one process drives all devices
    ShardGroup(data, device=d, rank=r, nranks=n, unique_id=b)   one process per GPU; rank 0 gets the
        128-byte id from ShardGroup.unique_id() and the caller broadcasts it (torch.distributed,
        MPI, a file ...).  unique_id=ShardGroup.PARTIAL_SUMS: no communicator, llk() returns this rank's
        partial sums (the caller reduces them); unique_id=None is accepted with nranks == 1 only."""

    PARTIAL_SUMS = "partial-sums"

    def __init__(self, data: PileupData, devices=None, device=0, rank=0, nranks=1, unique_id=None):
        self._lib = _abi.lib()
        self.data = data
        self.num_pc = data.num_pc
        inp = data.as_input()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            _abi.check(self._lib.vb2_shard_group_create(C.byref(inp), arr, len(devices), C.byref(h)),
                       "vb2_shard_group_create")
        else:
            if isinstance(unique_id, str) and unique_id == self.PARTIAL_SUMS:
                idbuf = C.c_void_p(1)                      # VB2_SHARD_PARTIAL_SUMS
            else:
                idbuf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), 128)
            _abi.check(self._lib.vb2_shard_group_create_rank(C.byref(inp), int(device), int(rank), int(nranks),
                                                             idbuf, C.byref(h)),
                       "vb2_shard_group_create_rank")
        self._h = h

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _abi.check(_abi.lib().vb2_rccl_unique_id(buf), "vb2_rccl_unique_id")
        return buf.raw

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vb2_shard_group_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        i = _abi.ShardInfo()
        _abi.check(self._lib.vb2_shard_group_info(self._h, C.byref(i)), "vb2_shard_group_info")
        n = i.num_shard
        return dict(num_shard=n, nranks=i.nranks, rank=i.rank, uses_rccl=bool(i.uses_rccl),
                    partial_sums=bool(i.partial_sums), rccl_stub=bool(i.rccl_stub),
                    num_allreduce=int(i.num_allreduce), marker_lo=list(i.marker_lo[:n]),
                    marker_hi=list(i.marker_hi[:n]), num_read=[int(x) for x in i.num_read[:n]])

    def llk(self, pc1, pc2, alpha):
        pc1 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc1, dtype=np.float64)))
        pc2 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc2, dtype=np.float64)))
        alpha = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)))
        B = alpha.shape[0]
        assert pc1.shape == (B, self.num_pc) and pc2.shape == (B, self.num_pc)
        out = np.zeros(B)
        _abi.check(self._lib.vb2_shard_group_eval(self._h, B, _p(pc1), _p(pc2), _p(alpha), _p(out)),
                   "vb2_shard_group_eval")
        return out

    def prepared_llk(self, pc1, pc2, alpha):
        """llk() with the argument marshalling done once: returns (step, out); step() makes one
        vb2_shard_group_eval call on the captured arrays (bench.py times steps, not numpy conversions)."""
        pc1 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc1, dtype=np.float64)))
        pc2 = np.ascontiguousarray(np.atleast_2d(np.asarray(pc2, dtype=np.float64)))
        alpha = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)))
        B = alpha.shape[0]
        assert pc1.shape == (B, self.num_pc) and pc2.shape == (B, self.num_pc)
        out = np.zeros(B)
        fn, h, a = self._lib.vb2_shard_group_eval, self._h, (_p(pc1), _p(pc2), _p(alpha), _p(out))

        def step(_keep=(pc1, pc2, alpha)):
            rc = fn(h, B, *a)
            if rc:
                _abi.check(rc, "vb2_shard_group_eval")
        return step, out

    def optimize(self, trace_capacity=0, **model_kw):
        m, keep = _model(known_af=self.data.known_af is not None, **model_kw)
        est = _abi.Estimate()
        tb = _TraceBuf(trace_capacity, self.num_pc) if trace_capacity else None
        _abi.check(self._lib.vb2_shard_group_optimize_llk(self._h, C.byref(m), C.byref(est),
                                                          C.byref(tb.c) if tb else None),
                   "vb2_shard_group_optimize_llk")
        out = _estimate_dict(est, self.num_pc)
        if tb:
            out["trace"], out["trace_count"] = tb.result()
        return out


def optimize_with_evaluator(evaluate, num_pc, trace_capacity=0, known_af=False, **model_kw):
    """OptimizeLLK over an arbitrary batched evaluator
        evaluate(pc1[B,k], pc2[B,k], alpha[B]) -> llk[B]
    (e.g. marker shards + an RCCL all-reduce).  The optimiser is the library's."""
    L = _abi.lib()
    k = int(num_pc)
    err = []

    def cb(_user, n, p1, p2, a, out):
        try:
            pc1 = np.ctypeslib.as_array(p1, (n, k)).copy()
            pc2 = np.ctypeslib.as_array(p2, (n, k)).copy()
            al = np.ctypeslib.as_array(a, (n,)).copy()
            res = np.asarray(evaluate(pc1, pc2, al), dtype=np.float64).reshape(n)
            np.ctypeslib.as_array(out, (n,))[:] = res
            return 0
        except Exception as exc:   # never let an exception cross the C boundary
            err.append(exc)
            return _abi.VB2_ERR_INVALID
    fn = _abi.EVAL_FN(cb)
    m, keep = _model(known_af=known_af, **model_kw)
    est = _abi.Estimate()
    tb = _TraceBuf(trace_capacity, k) if trace_capacity else None
    rc = L.vb2_optimize_llk(fn, None, k, C.byref(m), C.byref(est), C.byref(tb.c) if tb else None)
    if err:
        raise err[0]
    _abi.check(rc, "vb2_optimize_llk")
    out = _estimate_dict(est, k)
    if tb:
        out["trace"], out["trace_count"] = tb.result()
    return out


# the reference's defaults of its "Pileup Options" (main.cpp:81-96)
_MPILEUP_DEFAULTS = dict(min_bq=13, min_mq=2, adjust_mq=40, max_depth=8000, no_orphans=0, incl_flags=16 | 1024,
                         excl_flags=4 | 256 | 512 | 1024)


def _mpileup_opts(mpileup):
    """vb2_mpileup_opts from a dict of --min-BQ ... --excl-flags (names as in _MPILEUP_DEFAULTS); None = the defaults."""
    if mpileup is None:
        return _abi.MpileupOpts()
    unknown = set(mpileup) - set(_MPILEUP_DEFAULTS)
    if unknown:
        raise ValueError("unknown pileup option(s): %s" % sorted(unknown))
    o = dict(_MPILEUP_DEFAULTS, **mpileup)
    return _abi.MpileupOpts(1, *[int(o[n]) for n in ("min_bq", "min_mq", "adjust_mq", "max_depth", "no_orphans",
                                                      "incl_flags", "excl_flags")])


def _set_bam(args, bam_path, mpileup, apply_baq=False, reference_path=None):
    if bam_path is not None:
        if args.pileup_path is not None:
            raise ValueError("pileup_path and bam_path exclude each other")
        args.bam_path = str(bam_path).encode()
    args.mpileup = _mpileup_opts(mpileup)
    # --ApplyBAQ (vb2_run_args.bam_adjust): an int passes through as it is, so that a test can hand the library a value it refuses
    args.bam_adjust = int(apply_baq)
    if reference_path is not None:
        args.reference_path = str(reference_path).encode()


def run_files(svd_prefix, pileup_path, output_prefix=None, num_pc=2, disable_sanity=False,
              known_af_path=None, device=-1, output_pileup=False, devices=None, confidence_interval=False,
              per_chromosome=False, bootstrap=0, bam_path=None, mpileup=None, per_read_group=False, ref_bias=False,
              apply_baq=False, reference_path=None, fit_error=False, error_prior=0.0, error_table=None, **model_kw):
    """The --SVDPrefix/--PileupFile flow of execute() (vb2_run); devices=[a, b, ...] shards the
    sample's markers over those GPUs.  confidence_interval: vb2_run_interval (<output_prefix>.CI, and an
    `interval` entry in the result).  per_chromosome / bootstrap=N (seeded by seed=): vb2_run_replicates
    (<output_prefix>.Chrom / .Boot, and a `replicates` entry with the jackknife and bootstrap summaries).
    bam_path (with pileup_path=None): --BamFile through the built-in reader; mpileup: a dict of the reference's pileup
    options (min_bq, min_mq, adjust_mq, max_depth, no_orphans, incl_flags, excl_flags), None = its defaults.
    per_read_group (with bam_path): vb2_run_read_groups -- the whole sample as ever, <output_prefix>.selfRG, and a
    `read_groups` list in the result: per @RG line of the header its id, status (0, VB2_ERR_SANITY or 1 = no base), records,
    the estimate's entries (zero when not searched) and num_site, num_bases, avg_depth.
    ref_bias: vb2_run_refbias (<output_prefix>.RefBias, and a `ref_bias` entry in the result: the dict of RefBias.fit).
    apply_baq (with bam_path and reference_path, the FASTA with its .fai): --ApplyBAQ -- the Illumina shift, base alignment
    quality and the mapping-quality cap the pileup options ask for are applied to the records before the pileup.
    fit_error: vb2_run_errfit (<output_prefix>.ErrorFit and .ErrorRates, and an `error_fit` entry in the result: the dict of
    errfit); error_prior: the nominal rate's weight in pseudo-reads per quality, 0 = 100."""
    args, keep = _run_args(svd_prefix, pileup_path, num_pc, disable_sanity, known_af_path,
                           output_prefix, device, output_pileup, devices=devices, **model_kw)
    _set_bam(args, bam_path, mpileup, apply_baq, reference_path)
    res = _abi.RunResult()
    ci = _abi.Interval() if confidence_interval else None
    summary = None
    groups = None
    bias = None
    efit = None
    if error_table is not None:
        if fit_error or confidence_interval or per_chromosome or bootstrap or per_read_group or ref_bias:
            raise ValueError("error_table runs a plain run: it cannot be combined with fit_error, confidence_interval, per_chromosome, "
                             "bootstrap, per_read_group or ref_bias")
        table = _table_of(error_table)
        _abi.check(_abi.lib().vb2_run_under_table(C.byref(args), _p(table), C.byref(res)), "vb2_run_under_table")
    elif fit_error:
        if confidence_interval or per_chromosome or bootstrap or per_read_group or ref_bias:
            raise ValueError("fit_error cannot be combined with confidence_interval, per_chromosome, bootstrap, per_read_group "
                             "or ref_bias")
        efit = _abi.ErrFit()
        o = _errfit_opts(prior_reads=error_prior)
        _abi.check(_abi.lib().vb2_run_errfit(C.byref(args), C.byref(o), C.byref(res), C.byref(efit)), "vb2_run_errfit")
    elif ref_bias:
        if confidence_interval or per_chromosome or bootstrap or per_read_group:
            raise ValueError("ref_bias cannot be combined with confidence_interval, per_chromosome, bootstrap or per_read_group")
        bias = _abi.RefBiasFit()
        _abi.check(_abi.lib().vb2_run_refbias(C.byref(args), C.byref(res), C.byref(bias)), "vb2_run_refbias")
    elif per_read_group:
        if confidence_interval or per_chromosome or bootstrap:
            raise ValueError("per_read_group cannot be combined with confidence_interval, per_chromosome or bootstrap")
        L = _abi.lib()
        n = C.c_int32(0)
        cap = 64
        while True:
            buf = (_abi.GroupResult * cap)()
            _abi.check(L.vb2_run_read_groups(C.byref(args), C.byref(res), cap, buf, C.byref(n)), "vb2_run_read_groups")
            if n.value <= cap:
                break
            cap = n.value                     # (a header of more than 64 groups: once more with room for all)
        groups = []
        for g in buf[:n.value]:
            d = _estimate_dict(g.run.est, num_pc)
            d.update(status=int(g.status), header_index=int(g.header_index), records=int(g.records), num_site=g.run.num_site,
                     num_bases=int(g.run.num_bases), avg_depth=g.run.avg_depth, searched=g.status == _abi.VB2_OK,
                     seconds_optimize=g.run.seconds_optimize)
            groups.append(d)
    elif per_chromosome or bootstrap:
        if confidence_interval:
            raise ValueError("per_chromosome / bootstrap cannot be combined with confidence_interval")
        summary = _abi.ReplicateSummary()
        _abi.check(_abi.lib().vb2_run_replicates(C.byref(args), int(bool(per_chromosome)), int(bootstrap), C.byref(res),
                                                 C.byref(summary)), "vb2_run_replicates")
    elif ci is not None:
        _abi.check(_abi.lib().vb2_run_interval(C.byref(args), C.byref(res), C.byref(ci)), "vb2_run_interval")
    else:
        _abi.check(_abi.lib().vb2_run(C.byref(args), C.byref(res)), "vb2_run")
    out = _estimate_dict(res.est, num_pc)
    if ci is not None:
        out["interval"] = _interval_dict(ci)
    if summary is not None:
        out["replicates"] = {name: getattr(summary, name) for name, _ in _abi.ReplicateSummary._fields_}
    if groups is not None:
        out["read_groups"] = groups
    if bias is not None:
        out["ref_bias"] = _refbias_fit_dict(bias, num_pc)
    if efit is not None:
        out["error_fit"] = _errfit_dict(efit, num_pc)
    out.update(num_marker=res.num_marker, num_site=res.num_site, num_bases=int(res.num_bases),
               avg_depth=res.avg_depth, sd_depth=res.sd_depth, seconds_load=res.seconds_load,
               seconds_optimize=res.seconds_optimize)
    return out


def load_bam(svd_prefix, bam_path, num_pc=2, mpileup=None, device=-1, disable_sanity=True, known_af_path=None, apply_baq=False,
             reference_path=None):
    """vb2_flat_load of a BAM (the built-in reader: host stage, then the pileup on `device`), without a search: the
    panel-ordered reads -- read_off [M + 1], bases, quals as bytes --, num_site, num_bases, avg_depth and the load's
    vb2_bam_stats as `stats`.  apply_baq (with reference_path): --ApplyBAQ, and the stage's vb2_baq_stats as `baq`."""
    args, keep = _run_args(svd_prefix, None, num_pc, disable_sanity, known_af_path, None, device)
    _set_bam(args, bam_path, mpileup, apply_baq, reference_path)
    L = _abi.lib()
    h = C.c_void_p()
    _abi.check(L.vb2_flat_load(C.byref(args), C.byref(h)), "vb2_flat_load")
    try:
        inp = L.vb2_flat_input(h).contents
        M = inp.num_marker
        off = np.ctypeslib.as_array(C.cast(inp.read_off, C.POINTER(C.c_int64)), shape=(M + 1,)).copy()
        n = int(off[M])
        res = _abi.RunResult()
        _abi.check(L.vb2_flat_stats(h, C.byref(res)), "vb2_flat_stats")
        st = _abi.BamStats()
        _abi.check(L.vb2_flat_bam_stats(h, C.byref(st)), "vb2_flat_bam_stats")
        out = dict(read_off=off, bases=C.string_at(inp.bases, n) if n else b"", quals=C.string_at(inp.quals, n) if n else b"",
                   num_site=res.num_site, num_bases=int(res.num_bases), avg_depth=res.avg_depth,
                   stats={name: getattr(st, name) for name, _ in _abi.BamStats._fields_})
        if args.bam_adjust == 1:
            bs = _abi.BaqStats()
            _abi.check(L.vb2_flat_baq_stats(h, C.byref(bs)), "vb2_flat_baq_stats")
            out["baq"] = {name: getattr(bs, name) for name, _ in _abi.BaqStats._fields_}
        return out
    finally:
        L.vb2_flat_free(h)


def _flat_bam_dict(L, h):
    """read_off, bases, quals, num_site, num_bases, avg_depth of a vb2_flat"""
    inp = L.vb2_flat_input(h).contents
    M = inp.num_marker
    off = np.ctypeslib.as_array(C.cast(inp.read_off, C.POINTER(C.c_int64)), shape=(M + 1,)).copy()
    n = int(off[M])
    res = _abi.RunResult()
    _abi.check(L.vb2_flat_stats(h, C.byref(res)), "vb2_flat_stats")
    return dict(read_off=off, bases=C.string_at(inp.bases, n) if n else b"", quals=C.string_at(inp.quals, n) if n else b"",
                num_site=res.num_site, num_bases=int(res.num_bases), avg_depth=res.avg_depth)


def load_bam_groups(svd_prefix, bam_path, num_pc=2, mpileup=None, device=-1, disable_sanity=True, known_af_path=None,
                    apply_baq=False, reference_path=None):
    """vb2_flat_load_groups: the whole sample's dict as load_bam returns it, plus `groups` -- a list with one such dict (less
    `stats`) per @RG line of the header with its `id`, `records` and `status` --, `unassigned`, the number of kept records
    that belong to no group, and what the groups' part of the load took (groups_seconds_device, groups_seconds_copyback)."""
    args, keep = _run_args(svd_prefix, None, num_pc, disable_sanity, known_af_path, None, device)
    _set_bam(args, bam_path, mpileup, apply_baq, reference_path)
    L = _abi.lib()
    h, hg = C.c_void_p(), C.c_void_p()
    try:
        _abi.check(L.vb2_flat_load_groups(C.byref(args), C.byref(h), C.byref(hg)), "vb2_flat_load_groups")
        whole = _flat_bam_dict(L, h)
        st = _abi.BamStats()
        _abi.check(L.vb2_flat_bam_stats(h, C.byref(st)), "vb2_flat_bam_stats")
        whole["stats"] = {name: getattr(st, name) for name, _ in _abi.BamStats._fields_}
        groups = []
        for g in range(L.vb2_flat_groups_count(hg)):
            d = _flat_bam_dict(L, C.c_void_p(L.vb2_flat_groups_flat(hg, g)))
            d.update(id=L.vb2_flat_groups_id(hg, g).decode(), records=int(L.vb2_flat_groups_records(hg, g)),
                     status=int(L.vb2_flat_groups_status(hg, g)))
            groups.append(d)
        sd, sc = C.c_double(0), C.c_double(0)
        L.vb2_flat_groups_seconds(hg, C.byref(sd), C.byref(sc))
        whole.update(groups=groups, unassigned=int(L.vb2_flat_groups_unassigned(hg)), groups_seconds_device=sd.value,
                     groups_seconds_copyback=sc.value)
        return whole
    finally:
        if hg:
            L.vb2_flat_groups_free(hg)
        if h:
            L.vb2_flat_free(h)


def bam_scan(bam_path, bed_path, groups=False):
    """The built-in reader's host stage alone (vb2_bam_scan; no device): dict(voffsets -- the virtual offsets of the
    records it would send to the device, ascending --, sample, stats).  groups=True (vb2_bam_scan_ex with
    VB2_BAM_SCAN_GROUPS): also group_ids -- the header's @RG IDs in header order -- and record_groups, the records' group
    numbers parallel to voffsets (0xFFFF = none)."""
    L = _abi.lib()
    h = C.c_void_p()
    _abi.check(L.vb2_bam_scan_ex(str(bam_path).encode(), str(bed_path).encode(), _abi.VB2_BAM_SCAN_GROUPS if groups else 0,
                                 C.byref(h)), "vb2_bam_scan")
    try:
        n = L.vb2_bam_scan_records(h, None, 0)
        v = np.zeros(max(n, 1), dtype=np.uint64)
        L.vb2_bam_scan_records(h, v.ctypes.data_as(C.c_void_p), n)
        st = _abi.BamStats()
        L.vb2_bam_scan_stats(h, C.byref(st))
        out = dict(voffsets=v[:n], sample=L.vb2_bam_scan_sample(h).decode(),
                   stats={name: getattr(st, name) for name, _ in _abi.BamStats._fields_})
        if groups:
            ng = L.vb2_bam_scan_record_groups(h, None, 0)
            g = np.zeros(max(ng, 1), dtype=np.uint16)
            L.vb2_bam_scan_record_groups(h, g.ctypes.data_as(C.c_void_p), ng)
            out["group_ids"] = [L.vb2_bam_scan_group_id(h, i).decode() for i in range(L.vb2_bam_scan_num_group(h))]
            out["record_groups"] = g[:ng]
        return out
    finally:
        L.vb2_bam_scan_free(h)


def baq_records(bam_path, bed_path, reference_path, mpileup=None, where=0, device=-1):
    """vb2_baq_records: what --ApplyBAQ makes of the records the scan sends up, in its order.  where=0: the sequential host
    driver of csrc/baq_core.h (no device; a diagnostic, not a fallback), where=1: the device stage.  dict(qual_off [n + 1],
    qual (uint8, the adjusted qualities back to back), mapq (int16, -1 = dropped), outcome (uint8), cap4 [n, 4], stats)."""
    L = _abi.lib()
    h = C.c_void_p()
    opts = _mpileup_opts(mpileup)
    _abi.check(L.vb2_baq_records(str(bam_path).encode(), str(bed_path).encode(),
                                 None if reference_path is None else str(reference_path).encode(), C.byref(opts), int(where),
                                 int(device), C.byref(h)), "vb2_baq_records")
    try:
        n, nq = L.vb2_baq_result_num(h), L.vb2_baq_result_qual_bytes(h)
        off = np.zeros(n + 1, dtype=np.uint64)
        qual = np.zeros(max(nq, 1), dtype=np.uint8)
        mapq = np.zeros(max(n, 1), dtype=np.int16)
        outcome = np.zeros(max(n, 1), dtype=np.uint8)
        cap4 = np.zeros((max(n, 1), 4), dtype=np.int32)
        _abi.check(L.vb2_baq_result_copy(h, _p(off), _p(qual), _p(mapq), _p(outcome), _p(cap4)), "vb2_baq_result_copy")
        st = _abi.BaqStats()
        _abi.check(L.vb2_baq_result_stats(h, C.byref(st)), "vb2_baq_result_stats")
        return dict(qual_off=off, qual=qual[:nq], mapq=mapq[:n], outcome=outcome[:n], cap4=cap4[:n],
                    stats={name: getattr(st, name) for name, _ in _abi.BaqStats._fields_})
    finally:
        L.vb2_baq_result_free(h)


def baq_case(ref, query, qual, bw):
    """vb2_baq_case: the HMM of --ApplyBAQ alone on the host over codes 0..4: (state [int32], q [uint8], undefined rows)."""
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    query = np.ascontiguousarray(query, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    state = np.zeros(max(len(query), 1), dtype=np.int32)
    q = np.zeros(max(len(query), 1), dtype=np.uint8)
    und = C.c_int32(0)
    _abi.check(_abi.lib().vb2_baq_case(_p(ref) if len(ref) else None, len(ref), _p(query) if len(query) else None,
                                       _p(qual) if len(query) else None, len(query), int(bw), _p(state), _p(q), C.byref(und)),
               "vb2_baq_case")
    return state[:len(query)], q[:len(query)], und.value


def fasta_fetch(fasta_path, name, beg=0, end=None):
    """vb2_fasta_fetch: (nt16 codes of [beg, end) of the sequence as uint8, the sequence's length in the .fai)."""
    L = _abi.lib()
    length = C.c_int64(0)
    _abi.check(L.vb2_fasta_fetch(str(fasta_path).encode(), str(name).encode(), 0, 0, None, C.byref(length)), "vb2_fasta_fetch")
    if end is None:
        end = length.value
    out = np.zeros(max(end - beg, 1), dtype=np.uint8)
    _abi.check(L.vb2_fasta_fetch(str(fasta_path).encode(), str(name).encode(), int(beg), int(end), _p(out), C.byref(length)),
               "vb2_fasta_fetch")
    return out[:max(end - beg, 0)], length.value


def bgzf_inflate(data, device=-1):
    """The BGZF blocks of `data` (bytes: a whole file or any run of whole blocks) inflated on the device
    (vb2_bgzf_inflate: bgzf_inflate_kernel, one wave per block; no zlib fallback and no CRC32).  Returns (bytes, statuses):
    the blocks' bytes back to back -- zeros for a block the device refused -- and the device decoder's status per block
    (0 = inflated; the codes are in include/vb2_abi.h)."""
    L = _abi.lib()
    data = bytes(data)
    n_out, n_blk = C.c_int64(0), C.c_int32(0)
    # once without room, for the sizes (the block headers are checked first: a buffer that is not BGZF fails here)
    rc = L.vb2_bgzf_inflate(data, len(data), int(device), None, 0, C.byref(n_out), None, 0, C.byref(n_blk))
    if rc == _abi.VB2_OK:
        return b"", np.zeros(0, dtype=np.int32)
    if n_blk.value == 0:
        _abi.check(rc, "vb2_bgzf_inflate")
    status = np.zeros(n_blk.value, dtype=np.int32)
    out = np.zeros(max(n_out.value, 1), dtype=np.uint8)
    _abi.check(L.vb2_bgzf_inflate(data, len(data), int(device), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n_out),
                                  status.ctypes.data_as(C.c_void_p), status.size, C.byref(n_blk)), "vb2_bgzf_inflate")
    return out[:n_out.value].tobytes(), status[:n_blk.value].copy()


def bgzf_inflate_stats(reset=False):
    """vb2_bgzf_inflate_stats: what the device inflate of this process has done since the last reset, as a dict."""
    st = _abi.BgzfStats()
    _abi.check(_abi.lib().vb2_bgzf_inflate_stats(C.byref(st), int(bool(reset))), "vb2_bgzf_inflate_stats")
    return {name: getattr(st, name) for name, _ in _abi.BgzfStats._fields_}


def run_cohort_files(svd_prefix, pileup_paths, output_prefixes=None, num_pc=2, disable_sanity=False,
                     known_af_path=None, device=-1, output_pileup=False, group_size=0, num_host_thread=0,
                     devices=None, find_source=False, source_top=3, sources_prefix=None, confidence_interval=False,
                     refit_source=False, find_related=False, related_top=3, matched_normal=None, normal_hom_min=0.99,
                     pair_interval=False, mpileup=None, apply_baq=False, reference_path=None, cohort_fit_error=False,
                     pooled_error=False, error_prior=0.0, error_table=None, **model_kw):
    """Many pileups against one panel (vb2_cohort_run): the panel is read once, the pileups are read
    and flattened by host threads while the device searches the previous group in lock-step.
    Returns one dict per sample (with its own "status" code).
    A path that ends in ".bam" is read by the built-in BAM reader (its index beside it), with the pileup options of
    `mpileup` (as run_files'); lists may mix text pileups and BAMs.  The dict of a sample read from a BAM has a `bam` entry,
    the load's vb2_bam_stats.
    find_source (vb2_cohort_run_sources; one device): returns (samples, sources), sources = dict(score [S, S] -- row =
    target, column = candidate, NaN on the diagonal and for failed samples --, shared [S, S]); with output_prefixes and
    sources_prefix it writes <sources_prefix>.Sources, source_top candidates per sample.
    confidence_interval (vb2_cohort_run_intervals; one device; may be combined with find_source, which then returns no
    matrices: sources = None): every searched sample's dict has an `interval` entry, and with output_prefixes its
    <prefix>.CI is written.
    refit_source (with find_source; vb2_cohort_run_source_fits): sources also has `fit`, one dict per sample -- candidate
    (-1: none), markers, status (0: refitted, 1: no refit asked, < 0: the refit's error), llr, freemix, freelk1,
    alpha_given, lk1_given, lk0_given, delta_lk -- and <sources_prefix>.SourceFit is written.
    find_related (vb2_cohort_run_related; one device; may be combined with find_source, which then returns no score
    matrix; not with confidence_interval or refit_source): returns (samples, related), related = dict(llr [S, S, 4] in the
    order DUP, PO, FS, D2 -- row = target, column = partner --, shared [S, S]); with output_prefixes and sources_prefix it
    writes <sources_prefix>.Related, related_top partners per sample.
    matched_normal (vb2_cohort_run_paired; one device; with none of the above): a list of (tumour, normal) sample indices;
    returns (samples, fits), one dict per pair -- tumour, normal, markers, status (0: refitted, 1: the tumour or the normal
    failed its own run, < 0: the refit's error), normal_freemix, freemix, freelk1, alpha_paired, lk1_paired, lk0_paired --
    and with output_prefixes and sources_prefix <sources_prefix>.PairFit is written.  normal_hom_min: --NormalHomMin.
    pair_interval (with matched_normal; vb2_cohort_run_paired_intervals): every refitted pair's dict also has `interval` --
    alpha_paired unfolded in "freemix", its interval within [0, 1] -- and <sources_prefix>.PairCI is written.
    cohort_fit_error (vb2_cohort_run_errfit; one device; with none of the above): the error rates of every sample fitted in
    lock-step after the run, each on its own table or, with pooled_error, all on one; error_prior: --ErrorPrior.  Returns
    (samples, dict(fits=[the dict of errfit per sample], pool=the pooled summary)); with output_prefixes the per-sample
    <prefix>.ErrorFit / .ErrorRates, pooled with sources_prefix <sources_prefix>.ErrorRates / .PooledFit are written.
    error_table (vb2_cohort_run_under_table; with none of the above): a path in .ErrorRates format, or 94 rates -- the plain
    run with every sample's context under that table."""
    S = len(pileup_paths)
    if error_table is not None and (cohort_fit_error or find_source or find_related or confidence_interval or refit_source or
                                    matched_normal is not None):
        raise ValueError("error_table runs a plain cohort run: it cannot be combined with cohort_fit_error, find_source, find_related, "
                         "confidence_interval, refit_source or matched_normal")
    if pooled_error and not cohort_fit_error:
        raise ValueError("pooled_error needs cohort_fit_error")
    if cohort_fit_error and (find_source or find_related or confidence_interval or refit_source or matched_normal is not None):
        raise ValueError("cohort_fit_error cannot be combined with find_source, find_related, confidence_interval, refit_source or "
                         "matched_normal")
    if pair_interval and matched_normal is None:
        raise ValueError("pair_interval needs matched_normal")
    if matched_normal is not None and (find_source or find_related or confidence_interval or refit_source):
        raise ValueError("matched_normal cannot be combined with find_source, find_related, confidence_interval or refit_source")
    if find_related and (confidence_interval or refit_source):
        raise ValueError("find_related cannot be combined with confidence_interval or refit_source")
    if refit_source and (not find_source or confidence_interval):
        raise ValueError("refit_source needs find_source and cannot be combined with confidence_interval")
    args, keep = _run_args(svd_prefix, pileup_paths[0], num_pc, disable_sanity, known_af_path,
                           sources_prefix if find_source or find_related or matched_normal is not None or cohort_fit_error else None,
                           device, output_pileup, devices=devices, **model_kw)
    args.mpileup = _mpileup_opts(mpileup)
    args.bam_adjust = int(apply_baq)      # --ApplyBAQ for the list's .bam lines (reference_path: the FASTA)
    if reference_path is not None:
        args.reference_path = str(reference_path).encode()
    ca = _abi.CohortArgs()
    ca.base = args
    ca.num_sample = S
    piles = (C.c_char_p * S)(*[str(p).encode() for p in pileup_paths])
    ca.pileup_paths = piles
    prefs = None
    if output_prefixes is not None:
        prefs = (C.c_char_p * S)(*[str(p).encode() for p in output_prefixes])
        ca.output_prefixes = prefs
    ca.group_size = int(group_size)
    ca.num_host_thread = int(num_host_thread)
    res = (_abi.RunResult * S)()
    status = (C.c_int32 * S)()
    score = shared = None
    civ = None
    if error_table is not None:
        table = _table_of(error_table)
        _abi.check(_abi.lib().vb2_cohort_run_under_table(C.byref(ca), _p(table), res, status), "vb2_cohort_run_under_table")
    elif cohort_fit_error:
        efits, epool = (_abi.ErrFit * S)(), _abi.ErrFitPool()
        eo = _errfit_opts(error_prior)
        _abi.check(_abi.lib().vb2_cohort_run_errfit(C.byref(ca), C.byref(eo), int(bool(pooled_error)), res, status,
                                                    C.addressof(efits), C.addressof(epool)), "vb2_cohort_run_errfit")
    elif matched_normal is not None:
        pairs = np.ascontiguousarray(np.asarray(matched_normal, dtype=np.int32).reshape(-1, 2))
        tum, nrm = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        pfits = (_abi.PairFit * max(len(pairs), 1))()
        pci = (_abi.Interval * max(len(pairs), 1))()
        if pair_interval:
            _abi.check(_abi.lib().vb2_cohort_run_paired_intervals(C.byref(ca), len(pairs), _p(tum), _p(nrm), float(normal_hom_min),
                                                                  res, status, pfits, pci), "vb2_cohort_run_paired_intervals")
        else:
            _abi.check(_abi.lib().vb2_cohort_run_paired(C.byref(ca), len(pairs), _p(tum), _p(nrm), float(normal_hom_min), res,
                                                        status, pfits), "vb2_cohort_run_paired")
    elif find_related:
        llr, shared = np.zeros((S, S, _abi.VB2_NUM_RELATION)), np.zeros((S, S), dtype=np.int32)
        _abi.check(_abi.lib().vb2_cohort_run_related(C.byref(ca), int(related_top), int(source_top) if find_source else 0, res,
                                                     status, _p(llr), _p(shared)), "vb2_cohort_run_related")
    elif confidence_interval:
        civ = (_abi.Interval * S)()
        _abi.check(_abi.lib().vb2_cohort_run_intervals(C.byref(ca), int(source_top) if find_source else 0, res, status, civ),
                   "vb2_cohort_run_intervals")
    elif refit_source:
        score, shared = np.zeros((S, S)), np.zeros((S, S), dtype=np.int32)
        fits = (_abi.SourceFit * S)()
        _abi.check(_abi.lib().vb2_cohort_run_source_fits(C.byref(ca), int(source_top), res, status, _p(score), _p(shared), fits),
                   "vb2_cohort_run_source_fits")
    elif find_source:
        score, shared = np.zeros((S, S)), np.zeros((S, S), dtype=np.int32)
        _abi.check(_abi.lib().vb2_cohort_run_sources(C.byref(ca), int(source_top), res, status, _p(score), _p(shared)),
                   "vb2_cohort_run_sources")
    else:
        _abi.check(_abi.lib().vb2_cohort_run(C.byref(ca), res, status), "vb2_cohort_run")
    out = []
    for s in range(S):
        d = _estimate_dict(res[s].est, num_pc)
        d.update(status=int(status[s]), num_marker=res[s].num_marker, num_site=res[s].num_site,
                 num_bases=int(res[s].num_bases), avg_depth=res[s].avg_depth, sd_depth=res[s].sd_depth,
                 seconds_load=res[s].seconds_load, seconds_optimize=res[s].seconds_optimize)
        if civ is not None and status[s] == _abi.VB2_OK:
            d["interval"] = _interval_dict(civ[s])
        if str(pileup_paths[s]).endswith(".bam"):
            st = _abi.BamStats()
            if _abi.lib().vb2_cohort_bam_stats(s, C.byref(st)) == _abi.VB2_OK:
                d["bam"] = {name: getattr(st, name) for name, _ in _abi.BamStats._fields_}
        out.append(d)
    if cohort_fit_error:
        return out, dict(fits=[_errfit_dict(f, num_pc) for f in efits], pool=_errfit_pool_dict(epool))
    if matched_normal is not None:
        fits = [{name: getattr(pfits[p], name) for name, _ in _abi.PairFit._fields_} for p in range(len(pairs))]
        for p, f in enumerate(fits):
            if pair_interval and f["status"] == _abi.VB2_OK and pci[p].num_profile > 0:
                f["interval"] = _interval_dict(pci[p])
        return out, fits
    if find_related:
        return out, dict(llr=llr, shared=shared)
    if refit_source:
        fit = [{name: getattr(fits[s], name) for name, _ in _abi.SourceFit._fields_ if name != "reserved"} for s in range(S)]
        return out, dict(score=score, shared=shared, fit=fit)
    if find_source:
        return out, (None if civ is not None else dict(score=score, shared=shared))
    return out


# ---- reference-panel builder (--RefVCF): include/vb2_abi.h section 4 ----

PANEL_STAGES = ("parse", "upload", "gram", "centre", "eigensolve", "project", "write")


def _panel_args(vcf_path=None, num_svd_pcs=10, include_chr=None, skip_min_sample_count_check=False,
                check_minimums=False, num_thread=0, device=-1, notices=False, chunk_markers=0):
    a = _abi.PanelArgs()
    keep = []
    if vcf_path is not None:
        keep.append(str(vcf_path).encode())
        a.vcf_path = keep[-1]
    if include_chr is not None:   # a list of names or one comma-separated string; [] / "" = no chromosome filter
        s = include_chr if isinstance(include_chr, str) else ",".join(include_chr)
        keep.append(s.encode())
        a.include_chr = keep[-1]
    a.num_svd_pcs = int(num_svd_pcs)
    a.skip_min_sample_count_check = int(bool(skip_min_sample_count_check))
    a.check_minimums = int(bool(check_minimums))
    a.num_thread = int(num_thread)
    a.device = int(device)
    a.notices = int(bool(notices))
    a.chunk_markers = int(chunk_markers)
    return a, keep


def read_vcf(vcf_path, include_chr=None, num_thread=0, notices=False):
    """SVDcalculator::ReadVcf on the host (no device): the kept markers and their genotypes.

    include_chr=None is the reference's default (the 44 autosome names), [] keeps every chromosome.
    Returns a dict: genotypes (int8, markers x samples, -1 = missing), chr (list of str), pos (int32),
    ref, alt (lists of one-character str), samples (list of str)."""
    a, keep = _panel_args(vcf_path, include_chr=include_chr, num_thread=num_thread, notices=notices)
    L = _abi.lib()
    h = C.c_void_p()
    _abi.check(L.vb2_vcf_read(C.byref(a), C.byref(h)), "vb2_vcf_read")
    try:
        v = _abi.VcfView()
        _abi.check(L.vb2_vcf_get_view(h, C.byref(v)), "vb2_vcf_get_view")
        M, N = int(v.num_marker), int(v.num_sample)

        def arr(ptr, dtype, shape):
            if M == 0 or not ptr:
                return np.zeros(shape, dtype=dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape).copy()
        geno = arr(v.genotypes, np.int8, (M, N))
        pos = arr(v.pos, np.int32, (M,))
        ci = arr(v.chr_index, np.int32, (M,))
        ref = C.string_at(v.ref, M).decode("latin-1") if M else ""
        alt = C.string_at(v.alt, M).decode("latin-1") if M else ""
        names = [v.chr_names[i].decode() for i in range(v.num_chr)]
        samples = [v.sample_ids[i].decode() for i in range(N)]
    finally:
        L.vb2_vcf_free(h)
    return dict(genotypes=geno, chr=[names[i] for i in ci], pos=pos, ref=list(ref), alt=list(alt), samples=samples)


def _panel_result(h):
    L = _abi.lib()
    v = _abi.PanelView()
    _abi.check(L.vb2_panel_get_view(h, C.byref(v)), "vb2_panel_get_view")
    M, N, k = int(v.num_marker), int(v.num_sample), int(v.num_pc)

    def arr(ptr, ctype, shape):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape).copy()
    return dict(ud=arr(v.ud, C.c_double, (M, k)), v=arr(v.v, C.c_double, (N, k)), mu=arr(v.mu, C.c_double, (M,)),
                sigma=arr(v.sigma, C.c_double, (N,)), gram=arr(v.gram, C.c_int32, (N, N)),
                row_sum=arr(v.row_sum, C.c_int32, (M,)), num_pc=k,
                seconds=dict(zip(PANEL_STAGES, list(v.seconds))), seconds_total=v.seconds_total)


def build_panel(vcf_path, output_prefix=None, num_svd_pcs=10, include_chr=None, skip_min_sample_count_check=False,
                device=0, num_thread=0, notices=False, chunk_markers=0):
    """--RefVCF: read the VCF, decompose on the GPU, and (output_prefix given) write <prefix>.UD/.mu/.bed/.V in the
    reference's format -- the command line writes them at prefix = vcf_path.  Returns the arrays of _panel_result:
    ud (M x k), v (N x k), mu, sigma (full spectrum), gram (the exact int32 G^T G), row_sum, per-stage seconds."""
    a, keep = _panel_args(vcf_path, num_svd_pcs, include_chr, skip_min_sample_count_check, True, num_thread, device,
                          notices, chunk_markers)
    L = _abi.lib()
    h = C.c_void_p()
    _abi.check(L.vb2_panel_build(C.byref(a), C.byref(h)), "vb2_panel_build")
    try:
        if output_prefix is not None:
            _abi.check(L.vb2_panel_write(h, str(output_prefix).encode()), "vb2_panel_write")
        out = _panel_result(h)
    finally:
        L.vb2_panel_destroy(h)
    return out


def build_panel_from_genotypes(geno, num_svd_pcs=10, check_minimums=False, skip_min_sample_count_check=False,
                               device=0, notices=False, chunk_markers=0):
    """The same decomposition from an in-memory markers x samples matrix of -1/0/1/2 (PLINK-style sources, tests).
    The reference's minimums (5000 markers, 1000 samples) apply only with check_minimums=True."""
    g = np.ascontiguousarray(geno, dtype=np.int8)
    if g.ndim != 2:
        raise ValueError("geno must be a markers x samples matrix")
    a, keep = _panel_args(None, num_svd_pcs, None, skip_min_sample_count_check, check_minimums, 0, device, notices,
                          chunk_markers)
    L = _abi.lib()
    h = C.c_void_p()
    _abi.check(L.vb2_panel_build_genotypes(C.byref(a), g.ctypes.data, g.shape[0], g.shape[1], C.byref(h)),
               "vb2_panel_build_genotypes")
    try:
        out = _panel_result(h)
    finally:
        L.vb2_panel_destroy(h)
    return out
