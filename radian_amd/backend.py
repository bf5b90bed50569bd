"""Python face of the C ABI: one Backend == one rd_ctx == one GPU rank."""
import ctypes

import numpy as np

from . import _lib
from .weights import pack_blob, DEFAULT_DILATIONS

RD_TIMER_CONV, RD_TIMER_DECODE, RD_TIMER_HEAD, RD_TIMER_IN = 0, 1, 2, 3


class RadianHipError(RuntimeError):
    pass


def lib_path():
    return _lib.LIB_PATH


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


MISSING_CONTEXT = -1   # RD_LEN_MISSING_CONTEXT (include/radian_hip.h)


def _labels_of(labels, off, n):
    """one sequence's labels out of the flat label buffer -- or None where the library reports RD_LEN_MISSING_CONTEXT: the
    read's beam search looked up a context that the sparse RNA model does not hold (the reference raises KeyError there,
    radian/decode.py:83; radian_amd.basecall does when it reaches the read)"""
    if n == MISSING_CONTEXT:
        return None
    return labels[off: off + n].copy()


def device_count():
    """visible HIP devices (rd_device_count)"""
    n = ctypes.c_int(0)
    L = _lib.load()
    if L.rd_device_count(ctypes.byref(n)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return n.value


def device_for_rank(local_rank):
    """The device of a rank of a one-process-per-GPU job: its local rank -- or, when the launcher has narrowed every process's
    view (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES with fewer devices than local ranks), the local rank modulo what is visible."""
    n = device_count()
    if n < 1:
        raise RadianHipError("no HIP device is visible to this process")
    return local_rank if local_rank < n else local_rank % n


# rd_align_batch per-pair status (include/radian_hip.h RD_ALIGN_*)
ALIGN_OK, ALIGN_CLIP_INDEX_ERROR, ALIGN_EMPTY_AFTER_CLIP, ALIGN_TOO_LARGE = 0, 1, 2, 3
ALIGN_SCORES = (2, -4, -4, -2)   # radian/align.py:87: globalms(ref, seq, match, mismatch, gap open, gap extend)


# rd_ctc_align_batch per-sequence status (include/radian_hip.h RD_CTCALIGN_*)
CTCALIGN_OK, CTCALIGN_NO_PATH, CTCALIGN_TOO_LARGE = 0, 1, 2
CTCALIGN_STATUS_NAMES = ("ok", "no-path", "too-large")


def ctc_align_workspace_bytes(n_rows, n_labels):
    """device workspace Backend.ctc_align needs for one sequence of n_rows rows and n_labels labels (rd_ctc_align_workspace_bytes)"""
    return int(_lib.load().rd_ctc_align_workspace_bytes(int(n_rows), int(n_labels)))


class CtcAlignResult:
    """per sequence: first_step / last_step (int32 arrays, one entry per label), qual (uint8 array), score (float), status"""
    __slots__ = ("first_step", "last_step", "qual", "score", "status")

    def __init__(self, first_step, last_step, qual, score, status):
        self.first_step, self.last_step, self.qual, self.score, self.status = first_step, last_step, qual, score, status


class EventsResult:
    """per read, one entry per label: start / end (int32: the event's samples [start, end)), n = end - start, sum / sumsq (int64, over the raw
    int16 samples), min / max (int16).  A read without a path: start = end = -1 and zeros (rd_event_stats)"""
    __slots__ = ("start", "end", "n", "sum", "sumsq", "min", "max")

    def __init__(self, start, end, sum_, sumsq, min_, max_):
        self.start, self.end, self.sum, self.sumsq, self.min, self.max = start, end, sum_, sumsq, min_, max_
        self.n = [e - s for s, e in zip(start, end)]


def _event_buffers(tot):
    return (np.full(tot + 1, -1, dtype=np.int32), np.full(tot + 1, -1, dtype=np.int32), np.zeros(tot + 1, dtype=np.int64),
            np.zeros(tot + 1, dtype=np.int64), np.zeros(tot + 1, dtype=np.int16), np.zeros(tot + 1, dtype=np.int16))


def _events_of(bufs, cut):
    return EventsResult(*[[b[a:e].copy() for a, e in cut] for b in bufs])


def _event_args(raws, aln):
    flat, off = Backend._pack_raw(raws)
    n = len(raws)
    if not (len(aln.first_step) == len(aln.last_step) == len(aln.status) == n):
        raise ValueError(f"an alignment of {len(aln.status)} sequences for {n} reads")
    first = [np.ascontiguousarray(x, dtype=np.int32).ravel() for x in aln.first_step]
    last = [np.ascontiguousarray(x, dtype=np.int32).ravel() for x in aln.last_step]
    if any(a.shape != b.shape for a, b in zip(first, last)):
        raise ValueError("first_step and last_step differ in length")
    label_len = np.array([x.shape[0] for x in first], dtype=np.int32)
    label_off = np.zeros(n, dtype=np.int64)
    if n:
        label_off[1:] = np.cumsum(label_len[:-1].astype(np.int64))
    tot = int(label_len.astype(np.int64).sum())
    fbuf, lbuf = np.full(tot + 1, -1, dtype=np.int32), np.full(tot + 1, -1, dtype=np.int32)
    if tot:
        fbuf[:tot], lbuf[:tot] = np.concatenate(first), np.concatenate(last)
    status = np.ascontiguousarray(aln.status, dtype=np.int32)
    cut = [(int(label_off[i]), int(label_off[i] + label_len[i])) for i in range(n)]
    return flat, off, n, fbuf, lbuf, label_off, label_len, status, tot, cut


def event_stats_host(raws, aln):
    """Backend.event_stats on the host (rd_event_stats_host: the same boundary code and a plain loop; no GPU, no context)"""
    L = _lib.load()
    flat, off, n, fbuf, lbuf, label_off, label_len, status, tot, cut = _event_args(raws, aln)
    bufs = _event_buffers(tot)
    if L.rd_event_stats_host(_p(flat), _p(off), n, _p(fbuf), _p(lbuf), _p(label_off), _p(label_len), _p(status), *[_p(b) for b in bufs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _events_of(bufs, cut)


# rd_polya_segment per-read status (include/radian_hip.h RD_POLYA_*)
POLYA_OK, POLYA_NONE, POLYA_MAD_ZERO, POLYA_SHORT, POLYA_EMPTY, POLYA_TOO_LARGE = 0, 1, 2, 3, 4, 5
POLYA_STATUS_NAMES = ("ok", "none", "mad-zero", "short", "empty", "too-large")
POLYA_FIELDS = ("status", "tail_start", "tail_end", "n_flat", "sum", "sumsq", "m2", "d4", "n_candidates")


def polya_q(z):
    """a threshold of z in mad_normalise's units as the integer the C ABI takes (units of MAD / 256)"""
    return int(round(float(z) * 1.4826 * 256))


class PolyaParams:
    """rd_polya_segment's parameters, all integers (the contract is in include/radian_hip.h)"""
    __slots__ = ("win", "flat_q", "use_level", "lo_q", "hi_q", "max_gap", "min_samples", "search_limit")

    def __init__(self, win=32, flat_q=polya_q(0.12), use_level=0, lo_q=0, hi_q=0, max_gap=2, min_samples=480, search_limit=0):
        self.win, self.flat_q, self.use_level, self.lo_q, self.hi_q = int(win), int(flat_q), int(use_level), int(lo_q), int(hi_q)
        self.max_gap, self.min_samples, self.search_limit = int(max_gap), int(min_samples), int(search_limit)

    def args(self):
        return (self.win, self.flat_q, self.use_level, self.lo_q, self.hi_q, self.max_gap, self.min_samples, self.search_limit)


class PolyaResult:
    """one entry per read: status (int32, POLYA_*), tail_start / tail_end (int64 samples, -1 unless OK), n_flat (int32), sum / sumsq (int64
    over the samples of the tail), m2 / d4 (int32: twice the median, four times the MAD), n_candidates (int32)"""
    __slots__ = POLYA_FIELDS

    def __init__(self, n):
        for name in POLYA_FIELDS:
            setattr(self, name, np.zeros(n + 1, dtype=np.int64 if name in ("tail_start", "tail_end", "sum", "sumsq") else np.int32))

    def _bufs(self):
        return [_p(getattr(self, name)) for name in POLYA_FIELDS]

    def _cut(self, n):
        for name in POLYA_FIELDS:
            setattr(self, name, getattr(self, name)[:n])
        return self


def polya_segment_host(raws, params):
    """Backend.polya_segment on the host (rd_polya_segment_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    flat, off = Backend._pack_raw(raws)
    res = PolyaResult(len(raws))
    if L.rd_polya_segment_host(_p(flat), _p(off), len(raws), *params.args(), *res._bufs()) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return res._cut(len(raws))


def polya_workspace_bytes(n_samples, win):
    """device workspace Backend.polya_segment needs for one read (rd_polya_workspace_bytes)"""
    return int(_lib.load().rd_polya_workspace_bytes(int(n_samples), int(win)))


# rd_segment per-read status (include/radian_hip.h RD_SEGMENT_*)
SEGMENT_OK, SEGMENT_EMPTY, SEGMENT_TOO_LONG, SEGMENT_TOO_LARGE = 0, 1, 2, 3
SEGMENT_STATUS_NAMES = ("ok", "empty", "too-long", "too-large")
SEGMENT_EVENT_FIELDS = (("start", np.int32), ("sum", np.int64), ("sumsq", np.int64), ("min", np.int16), ("max", np.int16), ("src", np.uint8))


def segment_th(t):
    """a threshold on t as the integer the C ABI takes: t^2 in sixteenths"""
    return int(np.rint(16.0 * float(t) * float(t)))


class SegmentParams:
    """rd_segment's parameters, all integers (the contract is in include/radian_hip.h).  The defaults are `segment`'s."""
    __slots__ = ("w1", "w2", "th1", "th2", "v0")

    def __init__(self, w1=4, w2=12, th1=segment_th(2.5), th2=segment_th(5.0), v0=1):
        self.w1, self.w2, self.th1, self.th2, self.v0 = int(w1), int(w2), int(th1), int(th2), int(v0)

    def args(self):
        return (self.w1, self.w2, self.th1, self.th2, self.v0)


class SegmentResult:
    """status, n_events (int32 per read), m2 / d4 (int32 per read: the scale of the read's scale window, zeros without one) and per read a
    dict of its events' arrays: start (int32), sum / sumsq (int64), min / max (int16), src (uint8)"""
    __slots__ = ("status", "n_events", "m2", "d4", "events")


def _segment_call(fn, raws, params, scale_windows, extra):
    flat, off = Backend._pack_raw(raws)
    n = len(raws)
    room = [max(int(_lib.load().rd_segment_max_events(int(off[r + 1] - off[r]), params.w1)), 0) for r in range(n)]
    ev_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    res = SegmentResult()
    res.status, res.n_events, res.m2, res.d4 = (np.zeros(n + 1, np.int32) for _ in range(4))
    ev = [np.zeros(int(ev_off[-1]) + 1, dt) for _, dt in SEGMENT_EVENT_FIELDS]
    sc_lo = sc_hi = None
    if scale_windows is not None:
        sc_lo = np.array([off[r] + scale_windows[r][0] for r in range(n)] + [0], np.int64)
        sc_hi = np.array([off[r] + scale_windows[r][1] for r in range(n)] + [0], np.int64)
    rc = fn(_p(flat), _p(off), n, *params.args(), None if sc_lo is None else _p(sc_lo), None if sc_hi is None else _p(sc_hi), _p(ev_off), *extra,
            _p(res.status), _p(res.n_events), _p(res.m2), _p(res.d4), *[_p(a) for a in ev])
    res.status, res.n_events, res.m2, res.d4 = res.status[:n], res.n_events[:n], res.m2[:n], res.d4[:n]
    res.events = [{name: a[int(ev_off[r]):int(ev_off[r]) + int(res.n_events[r])].copy() for (name, _), a in zip(SEGMENT_EVENT_FIELDS, ev)}
                  for r in range(n)]
    return rc, res


def segment_host(raws, params, scale_windows=None):
    """Backend.segment on the host (rd_segment_host: the same rules in plain loops; no GPU, no context)"""
    L = _lib.load()
    rc, res = _segment_call(L.rd_segment_host, raws, params, scale_windows, ())
    if rc != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return res


def segment_workspace_bytes(n_samples, w1):
    """device workspace Backend.segment needs for one read (rd_segment_workspace_bytes)"""
    return int(_lib.load().rd_segment_workspace_bytes(int(n_samples), int(w1)))


def segment_max_events(n_samples, w1):
    """the event slots a read of n_samples needs (rd_segment_max_events)"""
    return int(_lib.load().rd_segment_max_events(int(n_samples), int(w1)))


# rd_site_compare per-site status (include/radian_hip.h RD_SITE_*)
SITE_OK, SITE_ONE_SIDED, SITE_DEEP, SITE_TOO_LARGE = 0, 1, 2, 3
SITE_STATUS_NAMES = ("ok", "one-sided", "deep", "too-large")
SITE_FIELDS = ("out_site", "status", "n", "sum", "sumsq", "vmin", "vmax", "med2", "u2", "ks_num", "ks_x", "tie")
_SITE_DTYPES = {"out_site": np.uint32, "status": np.int32, "n": np.int64, "sum": np.int64, "sumsq": np.int64, "vmin": np.int32, "vmax": np.int32,
                "med2": np.int32, "u2": np.int64, "ks_num": np.int64, "ks_x": np.int32, "tie": np.int64}
_SITE_PAIRS = ("n", "sum", "sumsq", "vmin", "vmax", "med2")


class SiteResult:
    """one entry per distinct site, ascending: out_site (uint32), status (int32, SITE_*), n / sum / sumsq (int64 [sites, 2]: sample 0 and
    1), vmin / vmax / med2 (int32 [sites, 2]; med2 is twice the median), u2 / ks_num / tie (int64), ks_x (int32).  include/radian_hip.h"""
    __slots__ = SITE_FIELDS

    def __init__(self, cap):
        for name in SITE_FIELDS:
            setattr(self, name, np.zeros((cap + 1, 2) if name in _SITE_PAIRS else cap + 1, dtype=_SITE_DTYPES[name]))

    def _bufs(self):
        return [_p(getattr(self, name)) for name in SITE_FIELDS]

    def _cut(self, n):
        for name in SITE_FIELDS:
            setattr(self, name, getattr(self, name)[:n])
        return self


def _site_args(site, cond, value, capacity):
    site = np.ascontiguousarray(site, dtype=np.uint32).ravel()
    cond = np.ascontiguousarray(cond, dtype=np.uint8).ravel()
    value = np.ascontiguousarray(value, dtype=np.int16).ravel()
    if not site.shape == cond.shape == value.shape:
        raise ValueError("site, cond and value differ in length")
    if capacity is None:
        capacity = int(np.unique(site).shape[0])
    return site, cond, value, int(capacity)


def site_compare_host(site, cond, value, n_sites, capacity=None):
    """Backend.site_compare on the host (rd_site_compare_host: the same rules over std::sort and plain loops; no GPU, no context)"""
    L = _lib.load()
    site, cond, value, capacity = _site_args(site, cond, value, capacity)
    res, n_out = SiteResult(capacity), ctypes.c_int64(0)
    if L.rd_site_compare_host(_p(site), _p(cond), _p(value), site.shape[0], int(n_sites), capacity, *res._bufs(), ctypes.byref(n_out)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return res._cut(n_out.value)


def site_workspace_bytes(n_events):
    """device workspace Backend.site_compare needs for a site of n_events events (rd_site_workspace_bytes)"""
    return int(_lib.load().rd_site_workspace_bytes(int(n_events)))


# rd_site_split (include/radian_hip.h): the statuses are SITE_* and SITE_NONE
SITE_NONE = 4
SPLIT_STATUS_NAMES = SITE_STATUS_NAMES + ("none",)
SPLIT_FIELDS = ("out_site", "status", "n", "sum", "sumsq", "cut", "n_cuts", "n_lo", "sum_lo", "sumsq_lo")
_SPLIT_DTYPES = {"out_site": np.uint32, "status": np.int32, "n": np.int64, "sum": np.int64, "sumsq": np.int64, "cut": np.int32, "n_cuts": np.int32,
                 "n_lo": np.int64, "sum_lo": np.int64, "sumsq_lo": np.int64}
_SPLIT_PAIRS = ("n", "sum", "sumsq", "n_lo", "sum_lo", "sumsq_lo")


class SplitResult:
    """one entry per distinct site, ascending: out_site (uint32), status (int32: SITE_* or SITE_NONE), n / sum / sumsq (int64 [sites, 2]:
    sample 0 and 1), cut / n_cuts (int32), n_lo / sum_lo / sumsq_lo (int64 [sites, 2]: each sample's values <= cut).  include/radian_hip.h"""
    __slots__ = SPLIT_FIELDS

    def __init__(self, cap):
        for name in SPLIT_FIELDS:
            setattr(self, name, np.zeros((cap + 1, 2) if name in _SPLIT_PAIRS else cap + 1, dtype=_SPLIT_DTYPES[name]))

    def _bufs(self):
        return [_p(getattr(self, name)) for name in SPLIT_FIELDS]

    def _cut(self, n):
        for name in SPLIT_FIELDS:
            setattr(self, name, getattr(self, name)[:n])
        return self


def site_split_host(site, cond, value, n_sites, min_frac_q16=0, capacity=None):
    """Backend.site_split on the host (rd_site_split_host: the same rules over std::sort and plain loops; no GPU, no context)"""
    L = _lib.load()
    site, cond, value, capacity = _site_args(site, cond, value, capacity)
    res, n_out = SplitResult(capacity), ctypes.c_int64(0)
    if L.rd_site_split_host(_p(site), _p(cond), _p(value), site.shape[0], int(n_sites), capacity, int(min_frac_q16), *res._bufs(),
                            ctypes.byref(n_out)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return res._cut(n_out.value)


def site_split_workspace_bytes(n_events):
    """device workspace Backend.site_split needs for a site of n_events events (rd_site_split_workspace_bytes)"""
    return int(_lib.load().rd_site_split_workspace_bytes(int(n_events)))


# rd_fit_batch per-query status (include/radian_hip.h RD_FIT_*)
FIT_OK, FIT_EMPTY, FIT_TOO_LARGE = 0, 1, 2


class FitResult:
    """Backend.fit_batch's per-query arrays: score, ref_start, ref_end int32 [n], counts int32 [n, 4] (n_match, n_sub, n_ins, n_del of
    the traced columns), status int32 [n] (FIT_*)."""

    def __init__(self, score, ref_start, ref_end, counts, status):
        self.score, self.ref_start, self.ref_end, self.counts, self.status = score, ref_start, ref_end, counts, status


# rd_sim_signal per-read status (include/radian_hip.h RD_SIM_*)
SIM_OK, SIM_EMPTY, SIM_TOO_LARGE = 0, 1, 2
SIM_STATUS_NAMES = ("ok", "empty", "too-large")


class SimModel:
    """rd_sim_*'s pore model, all integers (the contract is in include/radian_hip.h): k odd 1..9; level_q10, sd_q10, dwell_q8 int32 [4^k],
    indexed by the k-mer in pore order; dwell_cdf uint32 [1024]"""
    __slots__ = ("k", "level_q10", "sd_q10", "dwell_q8", "dwell_cdf")

    def __init__(self, k, level_q10, sd_q10, dwell_q8, dwell_cdf):
        self.k = int(k)
        self.level_q10 = np.ascontiguousarray(level_q10, dtype=np.int32).ravel()
        self.sd_q10 = np.ascontiguousarray(sd_q10, dtype=np.int32).ravel()
        self.dwell_q8 = np.ascontiguousarray(dwell_q8, dtype=np.int32).ravel()
        self.dwell_cdf = np.ascontiguousarray(dwell_cdf, dtype=np.uint32).ravel()
        n = 4 ** self.k if 1 <= self.k <= 9 else -1
        if not (self.level_q10.size == self.sd_q10.size == self.dwell_q8.size == n) or self.dwell_cdf.size != 1024:
            raise ValueError(f"a SimModel of k = {self.k} takes three tables of 4^k entries and 1024 dwell quantiles")

    def args(self):
        return (self.k, _p(self.level_q10), _p(self.sd_q10), _p(self.dwell_q8), _p(self.dwell_cdf))


class SimResult:
    """one entry per read: raw (int16 samples), base_first (int32: every base's first sample), status (int32, SIM_*)"""
    __slots__ = ("raw", "base_first", "status")

    def __init__(self, raw, base_first, status):
        self.raw, self.base_first, self.status = raw, base_first, status


def _sim_args(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale):
    """-> (the arrays, kept alive by the caller; the sixteen arguments every rd_sim_* entry point starts with; the base offsets)"""
    n = len(seqs)
    codes, off = _concat_codes(seqs)
    per = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32), (n,)) if np.ndim(a) == 0 else a, dtype=np.int32).ravel()
           for a in (lead, lead_level_q10, lead_sd_q10, median, scale_q10)]
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    if any(a.size != n for a in per) or keys.size != 2 * n:
        raise ValueError(f"per-read arguments that do not hold one entry for each of {n} reads (keys: two)")
    shift = dscale = None
    if level_shift is not None:
        shift, o = _pack(level_shift, np.int16, pad=1)
        if not np.array_equal(o, off):
            raise ValueError("level_shift does not hold one entry per base")
    if dwell_scale is not None:
        dscale, o = _pack(dwell_scale, np.uint16, pad=1)
        if not np.array_equal(o, off):
            raise ValueError("dwell_scale does not hold one entry per base")
    keep = (codes, off, per, keys, shift, dscale, model)
    return keep, (_p(codes), _p(off), n, _p(shift), _p(dscale), *[_p(a) for a in per], _p(keys), *model.args()), off


def _sim_result(raw, raw_off, bf, off, status, n):
    return SimResult([raw[raw_off[r]:raw_off[r + 1]].copy() for r in range(n)], [bf[off[r]:off[r + 1]].copy() for r in range(n)], status)


def sim_lengths_host(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift=None, dwell_scale=None):
    """Backend.sim_lengths on the host (rd_sim_lengths_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    keep, args, off = _sim_args(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
    out = np.zeros(len(seqs) + 1, dtype=np.int64)
    if L.rd_sim_lengths_host(*args, _p(out)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return out[:len(seqs)]


def sim_signal_host(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift=None, dwell_scale=None):
    """Backend.sim_signal on the host (rd_sim_signal_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    n = len(seqs)
    ns = sim_lengths_host(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
    keep, args, off = _sim_args(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
    raw_off = np.zeros(n + 1, dtype=np.int64)
    raw_off[1:] = np.cumsum(ns)
    raw, bf, status = np.zeros(int(raw_off[-1]) + 1, np.int16), np.zeros(int(off[-1]) + 1, np.int32), np.zeros(n + 1, np.int32)
    if L.rd_sim_signal_host(*args, _p(raw_off), _p(raw), _p(bf), _p(status)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _sim_result(raw, raw_off, bf, off, status[:n], n)


def sim_workspace_bytes(n_bases, n_samples):
    """device workspace Backend.sim_signal needs for one read (rd_sim_workspace_bytes); a launch adds sim_launch_bytes(k)"""
    return int(_lib.load().rd_sim_workspace_bytes(int(n_bases), int(n_samples)))


def sim_launch_bytes(k):
    """what a launch of Backend.sim_signal takes besides its reads: the model tables and the launch's own arrays (include/radian_hip.h)"""
    return (12 * 4 ** k + 4096 + 255) // 256 * 256 + 12288


# rd_eventalign per-read status (include/radian_hip.h RD_EVAL_*)
EVAL_OK, EVAL_EMPTY, EVAL_TOO_LONG, EVAL_MAD_ZERO, EVAL_NO_PATH, EVAL_TOO_LARGE, EVAL_OFF_BAND = 0, 1, 2, 3, 4, 5, 6
EVAL_STATUS_NAMES = ("ok", "empty", "too-long", "mad-zero", "no-path", "too-large", "off-band")
EVAL_BAND_W = 64   # states of rd_eventalign_banded's window (RD_EVAL_BAND_W)


class EvalModel:
    """rd_eventalign's pore model, all integers (the contract is in include/radian_hip.h): k odd 1..9; per k-mer in pore order lvl (int32,
    MAD/256), w (uint32, Q32 inverse variance), bias (int32, 1/32 nat); bg = (lvl, w, bias) of the background"""
    __slots__ = ("k", "lvl", "w", "bias", "bg")

    def __init__(self, k, lvl, w, bias, bg):
        self.k = int(k)
        self.lvl = np.ascontiguousarray(lvl, dtype=np.int32).ravel()
        self.w = np.ascontiguousarray(w, dtype=np.uint32).ravel()
        self.bias = np.ascontiguousarray(bias, dtype=np.int32).ravel()
        self.bg = (int(bg[0]), int(bg[1]), int(bg[2]))
        n = 4 ** self.k if 1 <= self.k <= 9 else -1
        if not (self.lvl.size == self.w.size == self.bias.size == n):
            raise ValueError(f"an EvalModel of k = {self.k} takes three tables of 4^k entries")

    def args(self):
        return (self.k, _p(self.lvl), _p(self.w), _p(self.bias), *self.bg)


class EvalResult:
    """per read: status (int32, EVAL_*), score (int64), m2 / d4 (int32: the scale as used), fit_sums (int64 [reads, 5]: N, sum l, sum l^2,
    sum x, sum x l); per read and base: first_step / last_step (int32 arrays, read sample coordinates) and events (an EventsResult)"""
    __slots__ = ("status", "score", "m2", "d4", "fit_sums", "first_step", "last_step", "events")

    def __init__(self, status, score, m2, d4, fit_sums, first_step, last_step, events):
        self.status, self.score, self.m2, self.d4, self.fit_sums = status, score, m2, d4, fit_sums
        self.first_step, self.last_step, self.events = first_step, last_step, events


def _eval_bases(seqs, n, per_read):
    """the bases side of both eventalign calls -> (codes, ref_off, ref_len, the per-base cut, the outputs: per_read's, first, last, events', fit sums)"""
    codes, coff = _concat_codes(seqs)
    tot = int(coff[-1])
    outs = [*[np.zeros(n + 1, dt) for dt in per_read], np.full(tot + 1, -1, np.int32), np.full(tot + 1, -1, np.int32), *_event_buffers(tot),
            np.zeros((n + 1, 5), np.int64)]
    ref_off = np.ascontiguousarray(coff[:-1] if n else np.zeros(1), dtype=np.int64)
    return codes, ref_off, np.diff(coff).astype(np.int32), [(int(coff[i]), int(coff[i + 1])) for i in range(n)], outs


def _eval_args(raws, seqs, model, t_lo, t_hi, m2, d4):
    """-> (the arrays, kept alive by the caller; the arguments up to the budget; the output buffers; the per-base cut)"""
    flat, off = Backend._pack_raw(raws)
    n = len(raws)
    if len(seqs) != n:
        raise ValueError(f"{len(seqs)} sequences for {n} reads")
    codes, ref_off, ref_len, cut, outs = _eval_bases(seqs, n, (np.int32, np.int64, np.int32, np.int32))
    lens = np.diff(off)
    lo = np.zeros(n, dtype=np.int64) if t_lo is None else np.ascontiguousarray(t_lo, dtype=np.int64).ravel()
    hi = lens.astype(np.int64) if t_hi is None else np.ascontiguousarray(t_hi, dtype=np.int64).ravel()
    m2 = np.zeros(n, dtype=np.int32) if m2 is None else np.ascontiguousarray(m2, dtype=np.int32).ravel()
    d4 = np.zeros(n, dtype=np.int32) if d4 is None else np.ascontiguousarray(d4, dtype=np.int32).ravel()
    if not (lo.size == hi.size == m2.size == d4.size == n):
        raise ValueError(f"per-read arguments that do not hold one entry for each of {n} reads")
    lo, hi, m2, d4 = (np.concatenate([a, np.zeros(1, a.dtype)]) for a in (lo, hi, m2, d4))   # (a pointer the library can check when n = 0)
    keep = (flat, off, codes, ref_off, ref_len, lo, hi, m2, d4, model)
    head = (_p(flat), _p(off), n, _p(lo), _p(hi), _p(codes), _p(ref_off), _p(ref_len), _p(m2), _p(d4), *model.args())
    return keep, head, outs, cut


def _eval_result(outs, cut, n):
    status, score, m2, d4, first, last = outs[:6]
    return EvalResult(status[:n], score[:n], m2[:n], d4[:n], outs[12][:n], [first[a:b].copy() for a, b in cut], [last[a:b].copy() for a, b in cut],
                      _events_of(outs[6:12], cut))


def eventalign_host(raws, seqs, model, t_lo=None, t_hi=None, m2=None, d4=None):
    """Backend.eventalign on the host (rd_eventalign_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    keep, head, outs, cut = _eval_args(raws, seqs, model, t_lo, t_hi, m2, d4)
    if L.rd_eventalign_host(*head, *[_p(b) for b in outs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _eval_result(outs, cut, len(raws))


def eventalign_workspace_bytes(n_rows, n_bases):
    """device workspace Backend.eventalign needs for one window of n_rows samples and n_bases bases (rd_eventalign_workspace_bytes)"""
    return int(_lib.load().rd_eventalign_workspace_bytes(int(n_rows), int(n_bases)))


class EvalBandedResult(EvalResult):
    """rd_eventalign_banded: an EvalResult (status may be EVAL_OFF_BAND) and n_edge (int32 per read: the bases whose rows touch the window's rim)"""
    __slots__ = ("n_edge",)


def _eval_banded_args(raws, seqs, guides, model, t_lo, t_hi, m2, d4):
    """_eval_args with the guide (one int32 array per read, one value per base, read sample coordinates) behind ref_len and n_edge behind d4"""
    keep, head, _, _ = _eval_args(raws, seqs, model, t_lo, t_hi, m2, d4)
    n = len(raws)
    if len(guides) != n or any(len(g) != len(q) for g, q in zip(guides, seqs)):
        raise ValueError("a guide holds one value for every base of its read")
    _, _, _, cut, outs = _eval_bases(seqs, n, (np.int32, np.int64, np.int32, np.int32, np.int32))
    guide = np.concatenate([np.ascontiguousarray(g, dtype=np.int32).ravel() for g in guides] + [np.zeros(1, np.int32)])
    return (keep, guide), (*head[:8], _p(guide), *head[8:]), outs, cut


def _eval_banded_result(outs, cut, n):
    base = _eval_result(outs[:4] + outs[5:], cut, n)
    res = EvalBandedResult(base.status, base.score, base.m2, base.d4, base.fit_sums, base.first_step, base.last_step, base.events)
    res.n_edge = outs[4][:n]
    return res


def eventalign_banded_host(raws, seqs, guides, model, t_lo=None, t_hi=None, m2=None, d4=None):
    """Backend.eventalign_banded on the host (rd_eventalign_banded_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    keep, head, outs, cut = _eval_banded_args(raws, seqs, guides, model, t_lo, t_hi, m2, d4)
    if L.rd_eventalign_banded_host(*head, *[_p(b) for b in outs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _eval_banded_result(outs, cut, len(raws))


def eventalign_banded_workspace_bytes(n_rows, n_bases):
    """device workspace Backend.eventalign_banded needs for one window of n_rows samples and n_bases bases (rd_eventalign_banded_workspace_bytes)"""
    return int(_lib.load().rd_eventalign_banded_workspace_bytes(int(n_rows), int(n_bases)))


# rd_modcall per-job status (include/radian_hip.h RD_MC_*)
MC_OK, MC_NO_ANCHOR, MC_NO_PATH, MC_TOO_LONG, MC_TOO_LARGE = 0, 1, 2, 3, 4
MC_STATUS_NAMES = ("ok", "no-anchor", "no-path", "too-long", "too-large")
MC_MAX_FLANK, MC_MAX_ALT, MC_MAX_ROWS = 27, 9, 1 << 15


class ModcallResult:
    """rd_modcall, per job (int32 arrays): status (MC_*), n_rows, n_states, vit_ref, vit_alt, fwd_ref, fwd_alt -- negative log likelihoods
    in 1/32 nat of the window's rows under the canonical states and with the job's entries in their place, by the best path and summed
    over all paths; zeros where status is not MC_OK.  llr() = (fwd_ref - fwd_alt) / 32 in nats (exact in float64)"""
    __slots__ = ("status", "n_rows", "n_states", "vit_ref", "vit_alt", "fwd_ref", "fwd_alt")

    def __init__(self, *arrays):
        self.status, self.n_rows, self.n_states, self.vit_ref, self.vit_alt, self.fwd_ref, self.fwd_alt = arrays

    def llr(self):
        return (self.fwd_ref.astype(np.int64) - self.fwd_alt) / 32.0


def _modcall_args(raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts, flank):
    """-> (the arrays, kept alive by the caller; the arguments up to the flank; the seven output buffers).  firsts / lasts: per read one
    int32 per base; alts: per job (lvl, w, bias), each of 1..9 entries"""
    flat, off = Backend._pack_raw(raws)
    n, nj = len(raws), len(job_read)
    if not (len(seqs) == len(firsts) == len(lasts) == n) or any(len(f) != len(q) or len(l) != len(q) for f, l, q in zip(firsts, lasts, seqs)):
        raise ValueError(f"modcall takes a sequence and one first and last step per base for each of {n} reads")
    if len(alt_first) != nj or len(alts) != nj:
        raise ValueError(f"modcall takes alt_first and the alt entries of each of {nj} jobs")
    codes, coff = _concat_codes(seqs)
    ref_off = np.ascontiguousarray(coff[:-1] if n else np.zeros(1), dtype=np.int64)
    ref_len = np.concatenate([np.diff(coff), np.zeros(1)]).astype(np.int32)
    def cat(xs, dt):      # (thousands of one-entry arrays: those that are already flat arrays of the type go in as they are)
        return np.concatenate([x if isinstance(x, np.ndarray) and x.dtype == dt and x.ndim == 1 else np.ascontiguousarray(x, dtype=dt).ravel() for x in xs]
                              + [np.zeros(1, dt)])
    first, last = cat(firsts, np.int32), cat(lasts, np.int32)
    m2, d4 = cat([m2], np.int32), cat([d4], np.int32)
    if m2.size != n + 1 or d4.size != n + 1:
        raise ValueError(f"modcall takes the scale of each of {n} reads")
    jr, af = cat([job_read], np.int32), cat([alt_first], np.int32)
    a_lvl, a_w, a_bias = cat([a[0] for a in alts], np.int32), cat([a[1] for a in alts], np.uint32), cat([a[2] for a in alts], np.int32)
    lens = [np.fromiter((np.size(a[i]) for a in alts), np.int64, nj) for i in range(3)]
    if not ((lens[0] == lens[1]).all() and (lens[0] == lens[2]).all()):
        raise ValueError("a job's alt entries are three arrays of one length")
    alt_off = np.zeros(nj + 1, np.int64)
    np.cumsum(lens[0], out=alt_off[1:])
    outs = [np.zeros(nj + 1, np.int32) for _ in range(7)]
    keep = (flat, off, m2, d4, codes, ref_off, ref_len, first, last, model, jr, af, alt_off, a_lvl, a_w, a_bias)
    head = (_p(flat), _p(off), n, _p(m2), _p(d4), _p(codes), _p(ref_off), _p(ref_len), _p(first), _p(last), model.k, _p(model.lvl), _p(model.w),
            _p(model.bias), nj, _p(jr), _p(af), _p(alt_off), _p(a_lvl), _p(a_w), _p(a_bias), int(flank))
    return keep, head, outs


def modcall_host(raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts, flank=6):
    """Backend.modcall on the host (rd_modcall_host: the same rules in a plain loop; no GPU, no context, no budget)"""
    L = _lib.load()
    keep, head, outs = _modcall_args(raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts, flank)
    if L.rd_modcall_host(*head, *[_p(b) for b in outs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return ModcallResult(*[b[:len(job_read)] for b in outs])


def modcall_workspace_bytes(n_samples, n_bases, n_jobs, n_alt):
    """device workspace Backend.modcall needs for one read: its samples, steps, jobs and alt entries (rd_modcall_workspace_bytes)"""
    return int(_lib.load().rd_modcall_workspace_bytes(int(n_samples), int(n_bases), int(n_jobs), int(n_alt)))


class EvalRowsResult:
    """rd_eventalign_events: per read status (int32, EVAL_*), score (int64), n_skipped (int32), m2 / d4 (int32: the scale as given), fit_sums
    (int64 [reads, 5]); per read and base: row_first / row_last (int32 arrays, indices into the read's events; -1 for a skipped base) and
    events (an EventsResult in read sample coordinates; start == end for a skipped base)"""
    __slots__ = ("status", "score", "n_skipped", "m2", "d4", "fit_sums", "row_first", "row_last", "events")


def _eval_rows_args(events, n_samples, seqs, model, m2, d4, sample_off, skip_pen):
    """-> (the arrays, kept alive by the caller; the arguments up to the budget; the output buffers; the per-base cut)"""
    n = len(events)
    if not (len(seqs) == len(n_samples) == len(m2) == len(d4) == n) or (sample_off is not None and len(sample_off) != n):
        raise ValueError(f"per-read arguments that do not hold one entry for each of {n} reads")
    codes, ref_off, ref_len, cut, outs = _eval_bases(seqs, n, (np.int32, np.int64, np.int32))
    cnt = np.array([len(e["start"]) for e in events] + [0], dtype=np.int32)
    ev_off = np.zeros(n + 1, dtype=np.int64)
    ev_off[1:] = np.cumsum(cnt[:n])
    ev = [np.concatenate([np.asarray(e[name], dtype=dt).ravel() for e in events] + [np.zeros(1, dt)])
          for name, dt in SEGMENT_EVENT_FIELDS if name != "src"]
    pad = lambda a, dt: np.concatenate([np.ascontiguousarray(a, dtype=dt).ravel(), np.zeros(1, dt)])   # (a pointer the library can check when n = 0)
    ns, so = pad(n_samples, np.int64), pad(np.zeros(n) if sample_off is None else sample_off, np.int64)
    m2, d4 = pad(m2, np.int32), pad(d4, np.int32)
    keep = (codes, ref_off, ref_len, cnt, ev_off, ev, ns, so, m2, d4, model)
    head = (n, _p(ns), _p(so), _p(ev_off), _p(cnt), *[_p(a) for a in ev], _p(codes), _p(ref_off), _p(ref_len), _p(m2), _p(d4), *model.args(),
            int(skip_pen))
    return keep, head, outs, cut


def _eval_rows_result(keep, outs, cut, n):
    res = EvalRowsResult()
    res.status, res.score, res.n_skipped = outs[0][:n], outs[1][:n], outs[2][:n]
    res.m2, res.d4 = keep[8][:n], keep[9][:n]
    res.row_first, res.row_last = [outs[3][a:b].copy() for a, b in cut], [outs[4][a:b].copy() for a, b in cut]
    res.events = _events_of(outs[5:11], cut)
    res.fit_sums = outs[11][:n]
    return res


def eventalign_events_host(events, n_samples, seqs, model, m2, d4, sample_off=None, skip_pen=96):
    """Backend.eventalign_events on the host (rd_eventalign_events_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    keep, head, outs, cut = _eval_rows_args(events, n_samples, seqs, model, m2, d4, sample_off, skip_pen)
    if L.rd_eventalign_events_host(*head, *[_p(b) for b in outs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _eval_rows_result(keep, outs, cut, len(events))


def eventalign_events_workspace_bytes(n_rows, n_bases):
    """device workspace Backend.eventalign_events needs for one read of n_rows events and n_bases bases (rd_eventalign_events_workspace_bytes)"""
    return int(_lib.load().rd_eventalign_events_workspace_bytes(int(n_rows), int(n_bases)))


# rd_sigmap per-query status (include/radian_hip.h RD_SIGMAP_*)
SIGMAP_OK, SIGMAP_EMPTY, SIGMAP_TOO_LONG, SIGMAP_MAD_ZERO, SIGMAP_NO_TARGET, SIGMAP_TOO_LARGE = 0, 1, 2, 3, 4, 5
SIGMAP_STATUS_NAMES = ("ok", "empty", "too-long", "mad-zero", "no-target", "too-large")
SIGMAP_MAX_T = 1 << 14     # rows of one query
SIGMAP_PAYLOAD = 6145      # end states one stripe of the DP kernel reports (csrc/sigmap_rules.h SM_PAYLOAD)
SIGMAP_BAND = 4096         # states of one workgroup pass (SM_BAND)


class SigmapResult:
    """per query: status (int32, SIGMAP_*), m2 / d4 (int32: the scale as used); per query and rank, int32 [queries, n_best], -1 past the
    number of targets: tgt (target index), score, end and org (the end and the origin state, local to the target)"""
    __slots__ = ("status", "m2", "d4", "tgt", "score", "end", "org")

    def __init__(self, status, m2, d4, tgt, score, end, org):
        self.status, self.m2, self.d4, self.tgt, self.score, self.end, self.org = status, m2, d4, tgt, score, end, org


class SigmapPanel:
    """a panel as rd_sigmap takes it: codes (uint8, 0..3, the targets end to end in pore order) and off (int64 [targets + 1], from 0)"""
    __slots__ = ("codes", "off")

    def __init__(self, codes, off):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8).ravel()
        self.off = np.ascontiguousarray(off, dtype=np.int64).ravel()
        if self.off.size == 0:
            raise ValueError("a SigmapPanel's offsets hold at least the 0 they start from")
        if self.codes.size == 0:
            self.codes = np.zeros(1, np.uint8)      # (a pointer the library can check)


def sigmap_panel(targets):
    """a sequence of uint8 code arrays, one per target (0..3, pore order) -> the SigmapPanel; a SigmapPanel is passed through.  (A pair of
    packed arrays is never guessed from a 2-tuple: two targets are two targets.)"""
    if isinstance(targets, SigmapPanel):
        return targets
    return SigmapPanel(*_pack(targets, np.uint8, pad=1))


def _sigmap_args(raw, targets, model, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best):
    """-> (the arrays, kept alive by the caller; the arguments up to n_best; the output buffers)"""
    raw = np.ascontiguousarray(raw, dtype=np.int16).ravel()
    n_raw = raw.size
    if n_raw == 0:
        raw = np.zeros(1, np.int16)
    pnl = sigmap_panel(targets)
    codes, off = pnl.codes, pnl.off
    q_lo = np.ascontiguousarray(q_lo, dtype=np.int64).ravel()
    n = q_lo.size
    R = int(off[-1])

    def per_query(a, default, dtype=np.int64):
        a = np.full(n, default, dtype=dtype) if a is None else np.ascontiguousarray(a, dtype=dtype).ravel()
        if a.size != n:
            raise ValueError(f"per-query arguments that do not hold one entry for each of {n} queries")
        return np.concatenate([a, np.zeros(1, dtype)])   # (a pointer the library can check when n = 0)

    q_hi = per_query(q_hi, 0)
    sc_lo = q_lo.copy() if sc_lo is None else sc_lo
    sc_hi = q_hi[:n].copy() if sc_hi is None else sc_hi
    arrs = [per_query(q_lo, 0), q_hi, per_query(sc_lo, 0), per_query(sc_hi, 0), per_query(m2, 0, np.int32), per_query(d4, 0, np.int32),
            per_query(s_lo, 0), per_query(s_hi, R)]
    nb = max(int(n_best), 1)
    outs = [np.zeros(n + 1, np.int32) for _ in range(3)] + [np.full((n + 1) * nb, -1, np.int32) for _ in range(4)]
    keep = (raw, codes, off, arrs, model)
    head = (_p(raw), n_raw, n, *[_p(a) for a in arrs], _p(codes), _p(off), off.size - 1, model.k, _p(model.lvl), _p(model.w), _p(model.bias), int(n_best))
    return keep, head, outs


def _sigmap_result(outs, n, n_best):
    return SigmapResult(outs[0][:n], outs[1][:n], outs[2][:n], *[o[:n * n_best].reshape(n, n_best) for o in outs[3:]])


def sigmap_host(raw, targets, model, q_lo, q_hi, sc_lo=None, sc_hi=None, m2=None, d4=None, s_lo=None, s_hi=None, n_best=1):
    """Backend.sigmap on the host (rd_sigmap_host: the same rules in a plain loop; no GPU, no context)"""
    L = _lib.load()
    keep, head, outs = _sigmap_args(raw, targets, model, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best)
    if L.rd_sigmap_host(*head, *[_p(b) for b in outs]) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return _sigmap_result(outs, head[2], int(n_best))


def sigmap_workspace_bytes(n_rows, n_states, n_tgt_in_range):
    """device workspace Backend.sigmap needs for one query of n_rows samples over n_states states that lie in n_tgt_in_range consecutive
    targets (rd_sigmap_workspace_bytes)"""
    return int(_lib.load().rd_sigmap_workspace_bytes(int(n_rows), int(n_states), int(n_tgt_in_range)))


def _pack(arrays, dtype, pad=0):
    """list of arrays -> (their elements as one flat buffer of dtype, int64 offsets [n + 1]); a buffer without elements has `pad` zeros (1
    where the library wants a pointer it can check)"""
    arrs = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([a.size for a in arrs])
    return (np.concatenate(arrs) if off[-1] else np.zeros(pad, dtype=dtype)), off


def _concat_codes(seqs):
    """list of code sequences (uint8 arrays / bytes / lists) -> (uint8 buffer, int64 offsets [n + 1])"""
    return _pack([np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else s for s in seqs], np.uint8, pad=1)


def _window_labels(labels, lens, nw):
    """chunk mode's label matrix [n_windows, chunk_len] and lengths [n_windows] -> per read (nw[r] windows) the list of its windows' label arrays"""
    out, w = [], 0
    for n in nw:
        out.append([labels[w + i, : lens[w + i]].copy() for i in range(n)])
        w += n
    return out


# rd_map_batch per-read status (include/radian_hip.h RD_MAP_*); MAP_EMPTY_SPAN is given by radian_amd.map, never by the library
MAP_OK, MAP_NO_SEED, MAP_NO_CHAIN, MAP_TOO_LARGE, MAP_EMPTY_SPAN = 0, 1, 2, 3, 4


class MapResult:
    """Backend.map_batch's per-read arrays, int32 [n] each: status (MAP_*), t, score, score2, n_anchors, q0, r0, q1, r1; stats: the
    call's counters (launches, minimizers, anchors, segments, stage_us) when asked for."""

    FIELDS = ("t", "score", "score2", "n_anchors", "q0", "r0", "q1", "r1")

    def __init__(self, status, hits, stats=None):
        self.status, self.hits, self.stats = status, hits, stats
        for c, name in enumerate(self.FIELDS):
            setattr(self, name, hits[:, c])


class CandResult:
    """Backend.map_candidates' per-read arrays: status (MAP_*), n_qual, n_cand int32 [n]; cands int32 [n, K, 8]: t, score, n_anchors, q0, r0,
    q1, r1, d3 of the read's candidates in (score descending, t ascending) order, rows past n_cand zero; stats as MapResult's, with the
    candidate stage under stage_us["candidates"]."""

    FIELDS = ("t", "score", "n_anchors", "q0", "r0", "q1", "r1", "d3")

    def __init__(self, status, n_qual, n_cand, cands, stats=None):
        self.status, self.n_qual, self.n_cand, self.cands, self.stats = status, n_qual, n_cand, cands, stats


QUANT_ONE = 1 << 20          # rd_quant_em's fixed point (csrc/quant_rules.h)
QUANT_MAX_W = 4096
QUANT_STATS = ("iterations", "last_delta", "lost", "reads_empty", "reads_single", "slots")


class QuantResult:
    """count uint64 [n_tx] and share uint32 [slots] (None when not asked for) in units of 2^-20 reads; stats: iterations, last_delta,
    lost, reads_empty, reads_single, slots, stage_us (upload, init, iterations, download; zeros from the host twin)."""

    def __init__(self, count, share, st):
        self.count, self.share = count, share
        self.stats = {nm: int(st[i]) for i, nm in enumerate(QUANT_STATS)}
        self.stats["stage_us"] = {nm: int(st[8 + i]) for i, nm in enumerate(("upload", "init", "iterations", "download"))}


def _quant_args(cand_off, cand_t, cand_w, n_tx, with_share):
    off = np.ascontiguousarray(cand_off, dtype=np.int64).reshape(-1)
    t = np.ascontiguousarray(cand_t, dtype=np.int32).reshape(-1)
    w_in = np.asarray(cand_w).reshape(-1)
    if w_in.size and (int(w_in.min()) < 0 or int(w_in.max()) > 65535):
        raise ValueError("quant_em: a weight does not fit 16 bits (1 .. 4096)")
    w = np.ascontiguousarray(w_in, dtype=np.uint16)
    if off.size < 1:
        raise ValueError("quant_em: cand_off needs n_reads + 1 entries")
    if t.size != w.size or (off.size and int(off.max(initial=0)) > t.size):
        raise ValueError("quant_em: cand_off ends beyond cand_t / cand_w, or the two differ in length")
    count = np.zeros(max(int(n_tx), 1), dtype=np.uint64)
    share = np.zeros(max(t.size, 1), dtype=np.uint32) if with_share else None
    pad = lambda a, dt: a if a.size else np.zeros(1, dtype=dt)
    return off, pad(t, np.int32), pad(w, np.uint16), t.size, count, share


def quant_em_host(cand_off, cand_t, cand_w, n_tx, max_iter=1000, tol_q20=1024, with_share=True):
    """Backend.quant_em on the host (rd_quant_em_host: the same rules and packed form in plain loops; no GPU, no context)"""
    L = _lib.load()
    off, t, w, slots, count, share = _quant_args(cand_off, cand_t, cand_w, n_tx, with_share)
    st = np.zeros(16, dtype=np.int64)
    if L.rd_quant_em_host(_p(off), _p(t), _p(w), off.size - 1, int(n_tx), int(max_iter), int(tol_q20), _p(count), _p(share), _p(st)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return QuantResult(count[:int(n_tx)], None if share is None else share[:slots], st)


# rd_diag_score_math's routines (include/radian_hip_diag.h RD_SM_*): 0..3 and 10 exist on the device only
(SM_EXP_NONPOS, SM_LOG1P_UNIT, SM_LAE, SM_SAFE_LOG, SM_GM_EXP, SM_GM_LOG, SM_GM_LOG1P, SM_GM_LOG1P_UNIT, SM_LAE_GX, SM_SAFE_LOG_GX,
 SM_COUNT4_GT) = range(11)


def _score_math_args(which, x, y):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    n = x.size // 4 if which == SM_COUNT4_GT else x.size
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if y.size != n or (which == SM_COUNT4_GT and x.size != 4 * n):
            raise ValueError("score_math: x and y differ in length (count4_gt: x holds four keys per entry of y)")
        if n == 0:
            y = np.zeros(1, dtype=np.float64)
    return (x if x.size else np.zeros(4, dtype=np.float64)), y, n


def score_math_host(which, x, y=None):
    """Backend.score_math on the host (rd_diag_score_math_host: the glibc routines, SM_GM_EXP .. SM_SAFE_LOG_GX, from the same header
    compiled for the host; no GPU, no context)"""
    L = _lib.load()
    x, y, n = _score_math_args(which, x, y)
    out = np.zeros(max(n, 1), dtype=np.float64)
    if L.rd_diag_score_math_host(int(which), _p(x), _p(y), n, _p(out)) != 0:
        raise RadianHipError(L.rd_last_error().decode())
    return out[:n]


def quant_workspace_bytes(slots, n_reads, n_tx):
    """an upper bound of the device workspace Backend.quant_em reserves (rd_quant_workspace_bytes)"""
    return int(_lib.load().rd_quant_workspace_bytes(int(slots), int(n_reads), int(n_tx)))


def map_minimizers(codes, k, w):
    """(positions int32, hashes uint32) of the (w,k)-minimizers of one record of codes (0..3; anything else a break): the library's
    own seed code on the host (rd_map_minimizers; no GPU)."""
    L = _lib.load()
    c = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    n = c.size
    buf = c if n else np.zeros(1, dtype=np.uint8)
    pos = np.zeros(max(n, 1), dtype=np.int32)
    hs = np.zeros(max(n, 1), dtype=np.uint32)
    got = ctypes.c_int64(0)
    rc = L.rd_map_minimizers(_p(buf), n, int(k), int(w), _p(pos), _p(hs), pos.size, ctypes.byref(got))
    if rc != 0:
        raise RadianHipError(f"[rd error {rc}] " + L.rd_last_error().decode("utf-8", "replace"))
    return pos[: got.value].copy(), hs[: got.value].copy()


def tfrecord_write(path, signals, input_len, labels, label_len=None, append=False):
    """Write labelled windows as a TFRecord shard of tf.train.Example records (radian/data.py:9-15), the library's rd_tfrecord_write
    (host; no GPU).  signals float32 [n, 1024], input_len [n] (signal_length, 1..1024), labels as Backend.ctc_eval takes them."""
    L = _lib.load()
    sig = np.ascontiguousarray(signals, dtype=np.float32)
    n = len(input_len)
    if sig.size != n * CTC_T:
        raise ValueError(f"signals must be [{n}, {CTC_T}] float32")
    il = np.ascontiguousarray(input_len, dtype=np.int32).reshape(-1)
    buf, off, ll = _pack_labels(labels, label_len, n)
    rc = L.rd_tfrecord_write(str(path).encode(), _p(sig), _p(il), _p(buf), _p(off), _p(ll), n, 1 if append else 0)
    if rc == -7:
        raise OSError(L.rd_last_error().decode("utf-8", "replace"))
    if rc != 0:
        raise RadianHipError(f"[rd error {rc}] " + L.rd_last_error().decode("utf-8", "replace"))


def _as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def _concat(seqs):
    """bytes of a list of str / bytes -> (uint8 buffer, int64 offsets [n + 1])"""
    bs = [_as_bytes(s) for s in seqs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    buf = np.frombuffer(b"".join(bs), dtype=np.uint8) if off[-1] else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), off


def align_workspace_bytes(n, m):
    """device workspace (bytes) rd_align_batch needs for one n x m pair alone (rd_align_workspace_bytes; no GPU)"""
    return int(_lib.load().rd_align_workspace_bytes(int(n), int(m)))


def align_clip_count(ops, ref, read):
    """analyse_alignment's soft clip and counts (radian/align.py:9-57) of one alignment given as its column ops (M / X / D / I)
    and the characters its D / I columns consume -- the library's own code (rd_align_clip_count, host; no GPU).
    Returns ((n_match, n_sub, n_ins, n_del), status)."""
    L = _lib.load()
    o, r, q = (np.frombuffer(_as_bytes(x), dtype=np.uint8) if len(x) else np.zeros(1, dtype=np.uint8) for x in (ops, ref, read))
    cnt = np.zeros(4, dtype=np.int32)
    st = np.zeros(1, dtype=np.int32)
    rc = L.rd_align_clip_count(_p(o), len(ops), _p(r), _p(q), _p(cnt), _p(st))
    if rc != 0:
        raise RadianHipError(f"[rd error {rc}] " + L.rd_last_error().decode("utf-8", "replace"))
    return tuple(int(c) for c in cnt), int(st[0])


class AlignResult:
    """Backend.align's per-pair arrays: score int32 [n], counts int32 [n, 4] (n_match, n_sub, n_ins, n_del after the soft clip),
    status int32 [n] (ALIGN_*), ops (list of bytes of M / X / D / I columns, or None when not asked for)."""

    def __init__(self, score, counts, status, ops):
        self.score, self.counts, self.status, self.ops = score, counts, status, ops


# rd_pileup_* (include/radian_hip.h RD_PILEUP_*)
PILEUP_OK, PILEUP_NO_BASE, PILEUP_TOO_LARGE = 0, 1, 2
PILEUP_CHANNELS = ("A", "C", "G", "T", "other", "del", "ins", "starts")
PILEUP_FIELDS = ("status", "score", "ref_lo", "ref_hi", "clip_head", "clip_tail", "n_match", "n_sub", "n_ins", "n_del")
PILEUP_CONF, PILEUP_INS_BASE, PILEUP_KMER, PILEUP_INS_LEN, PILEUP_DEL_LEN, PILEUP_PROFILE_LEN = 0, 30, 35, 4131, 4195, 4259


class PileupPairs:
    """Per-pair results of Backend.pileup_add / pileup_add_ops / pileup_host: out int32 [n, 10] (PILEUP_FIELDS: the counts are those of
    the covered interval, not Backend.align's), every field also as an attribute; ops (list of bytes, or None when not asked for)."""

    def __init__(self, out, ops=None):
        self.out, self.ops = out, ops
        for i, nm in enumerate(PILEUP_FIELDS):
            setattr(self, nm, out[:, i])


class PileupTable:
    """Backend.pileup_read: site uint32 [n_out] (ascending), counts uint32 [n_out, 8] (PILEUP_CHANNELS), profile uint64 [PILEUP_PROFILE_LEN]"""

    def __init__(self, site, counts, profile):
        self.site, self.counts, self.profile = site, counts, profile


def _pileup_args(refs, reads, site0, ops=None):
    n = len(refs)
    if len(reads) != n or len(site0) != n or (ops is not None and len(ops) != n):
        raise ValueError(f"{len(refs)} spans, {len(reads)} reads, {len(site0)} sites" + ("" if ops is None else f", {len(ops)} op strings"))
    rbuf, roff = _concat(refs)
    qbuf, qoff = _concat(reads)
    s0 = np.ascontiguousarray(np.asarray(site0, dtype=np.int64).reshape(-1)) if n else np.zeros(1, dtype=np.int64)
    out = np.zeros((max(n, 1), 10), dtype=np.int32)
    obuf, ooff = _concat(ops) if ops is not None else (None, None)
    return n, rbuf, roff, qbuf, qoff, s0, out, obuf, ooff


def pileup_host(ops, refs, reads, site0, n_sites, sites=None, profile=None):
    """The pileup rules on the host (rd_pileup_host: plain loops; no GPU, no context), ADDED into sites uint32 [n_sites, 8] and profile
    uint64 [PILEUP_PROFILE_LEN] (fresh zeroed tables when None).  Returns (PileupPairs, sites, profile)."""
    L = _lib.load()
    n, rbuf, roff, qbuf, qoff, s0, out, obuf, ooff = _pileup_args(refs, reads, site0, ops)
    if sites is None:
        sites = np.zeros((max(int(n_sites), 1), 8), dtype=np.uint32)
    if profile is None:
        profile = np.zeros(PILEUP_PROFILE_LEN, dtype=np.uint64)
    if sites.dtype != np.uint32 or profile.dtype != np.uint64 or not sites.flags.c_contiguous or sites.size < 8 * int(n_sites) or profile.size < PILEUP_PROFILE_LEN:
        raise ValueError("pileup_host: sites is uint32 [n_sites, 8], profile uint64 [PILEUP_PROFILE_LEN]")
    rc = L.rd_pileup_host(_p(obuf), _p(ooff), _p(rbuf), _p(roff), _p(qbuf), _p(qoff), n, _p(s0), int(n_sites), _p(sites), _p(profile), _p(out))
    if rc != 0:
        raise RadianHipError(f"[rd error {rc}] " + L.rd_last_error().decode("utf-8", "replace"))
    return PileupPairs(out[:n]), sites, profile


def pileup_workspace_bytes(n, m):
    """device workspace (bytes) rd_pileup_add needs for one n x m pair alone (rd_pileup_workspace_bytes; no GPU)"""
    return int(_lib.load().rd_pileup_workspace_bytes(int(n), int(m)))


# rd_ctc_* per-window status (include/radian_hip.h RD_CTC_*)
CTC_OK, CTC_INFEASIBLE = 0, 1
CTC_T, CTC_MAX_LABEL = 1024, 255


def _pack_labels(labels, label_len, n):
    """labels: [n, Lmax] array (Keras's dense form) or a list of n sequences, label_len: counted labels of each (None: all of a
    sequence) -> (uint8 buffer, int64 offsets [n], int32 lengths [n])"""
    if label_len is None:
        label_len = [len(l) for l in labels]
    ll = np.ascontiguousarray(label_len, dtype=np.int32).reshape(-1)
    if len(labels) != n or ll.size != n:
        raise ValueError(f"{len(labels)} label rows and {ll.size} lengths for {n} windows")
    rows = []
    for i in range(n):
        row = np.asarray(labels[i]).reshape(-1)
        if ll[i] < 0 or ll[i] > row.size:
            raise ValueError(f"window {i}: label_length {int(ll[i])} outside 0..{row.size}")
        r = row[: ll[i]]
        if r.size and (np.any(r != np.round(r)) or r.min() < 0 or r.max() > 3):
            raise ValueError(f"window {i}: labels must be 0..3")
        rows.append(r.astype(np.uint8))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ll, out=off[1:])
    buf = np.concatenate(rows) if off[-1] else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), np.ascontiguousarray(off[:-1]), ll


class CtcResult:
    """Backend.ctc_eval / ctc_probs per-window arrays: loss float64 [n] (+inf when infeasible), status int32 [n] (CTC_*),
    greedy_len int32 [n], edit_distance int32 [n], greedy (list of uint8 arrays, or None when not asked for)."""

    def __init__(self, loss, status, greedy_len, edit_distance, greedy):
        self.loss, self.status, self.greedy_len, self.edit_distance, self.greedy = loss, status, greedy_len, edit_distance, greedy


class PipeTicket:
    """One batch queued on a Backend's pipeline (Backend.pipe_submit_raw).  The arrays the library writes into
    live here until the batch is delivered."""

    def __init__(self, be, decode_type, off, n):
        self.be, self.decode_type, self.off, self.n = be, decode_type, off, n
        self.status = np.zeros(n, dtype=np.int32)
        self.labels = self.lens = self.label_off = self.nw = None
        self.seq = 0

    def done(self):
        return self.be.pipe_progress(0) >= self.seq

    def wait(self):
        if self.be.pipe_progress(self.seq) < self.seq:
            raise RadianHipError("pipeline did not deliver the awaited batch")

    def result_raw(self):
        """chunk mode, blocks until delivered: (label matrix uint8 [n_windows, chunk_len], lengths int32 [n_windows], windows
        per read, status) -- what radian_amd.sequence_assembly.consensus_batch takes, without a Python object per window"""
        self.wait()
        return self.labels, self.lens, self.nw, self.status

    def result(self):
        """(labels, status) as basecall_raw_global / basecall_raw_chunk return them; blocks until delivered"""
        self.wait()
        if self.decode_type == "global":
            return [_labels_of(self.labels, self.off[r], self.lens[r]) for r in range(self.n)], self.status
        return _window_labels(self.labels, self.lens, self.nw), self.status


class Backend:
    """Owns an rd_ctx.  All compute goes to the HIP library; nothing here falls back to the CPU."""

    def __init__(self, device_id=0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        self._h = None
        self._check(self._L.rd_create(int(device_id), ctypes.byref(h)))
        self._h = h
        self.device_id = device_id
        self.lm_k = None
        # undelivered PipeTickets by submit number: the library writes a batch's labels / lengths / status into the ticket's
        # arrays when it DELIVERS the batch (rd_pipe_progress / rd_pipe_flush, possibly on behalf of another ticket's wait),
        # so the arrays must outlive a ticket the caller dropped
        self._tickets = {}

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise RadianHipError(f"[rd error {rc}] " + self._L.rd_last_error().decode("utf-8", "replace"))

    def close(self):
        if self._h is not None:
            self._L.rd_destroy(self._h)      # (does not deliver: nothing is written into ticket arrays after this)
            self._h = None
        self._tickets.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self._L.rd_sync(self._h))

    def set_precision(self, mode):
        """'fp32' (default, exact fp32 MFMA), 'f16x3' (split-f16 matrix products, 22-bit operands) or 'bf16x3' (three-term
        bf16 split: every fp32 operand exact, six bf16 MFMAs per product)."""
        code = {"fp32": 0, "f16x3": 1, "bf16x3": 2}[mode] if isinstance(mode, str) else int(mode)
        self._check(self._L.rd_set_precision(self._h, code))

    def set_conv_shape(self, shape):
        """0 (default): 128-row tiles, two 256-thread workgroups per CU; 1: 256-row tiles, one 512-thread workgroup per CU (fp32 mode)."""
        self._check(self._L.rd_set_conv_shape(self._h, int(shape)))

    def split3(self, values):
        """Device-side three-term bf16 split of float32 values -> uint16 [3, n] bit patterns (hi, mid, lo)."""
        v = np.ascontiguousarray(values, dtype=np.float32).ravel()
        out = np.zeros((3, v.size), dtype=np.uint16)
        self._check(self._L.rd_split3(self._h, _p(v), v.size, _p(out)))
        return out

    @property
    def max_beam_width(self):
        return self._L.rd_decode_max_width()

    # ------------------------------------------------------------------ artefacts
    def load_weights(self, flat, dilations=DEFAULT_DILATIONS):
        """model.load_weights (radian/model.py:44): flat float32 parameters in Keras order."""
        blob = pack_blob(flat, dilations)
        self.load_weights_blob(blob)

    def load_weights_blob(self, blob):
        buf = ctypes.create_string_buffer(blob, len(blob))
        self._check(self._L.rd_load_weights(self._h, ctypes.cast(buf, ctypes.c_void_p), len(blob)))

    def load_lm(self, table, k):
        """LM table [4^k,4] float64 (radian/basecall.py:48-57); rows of NaN mark contexts a sparse model does not hold
        (lm.table_from_dict); None unloads."""
        if table is None:
            self._check(self._L.rd_load_lm(self._h, None, 0))
            self.lm_k = None
            return
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.shape != (4 ** k, 4):
            raise ValueError(f"LM table must be [4^{k},4], got {table.shape}")
        self._check(self._L.rd_load_lm(self._h, _p(table), int(k)))
        self.lm_k = k

    UNSEEN = {"backoff": 0, "uniform": 1, "absent": 2}

    @staticmethod
    def _records(codes, offsets):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1 or codes.ndim != 1 or int(offsets[-1]) != len(codes):
            raise ValueError("offsets must be [records + 1] and end at len(codes)")
        return (codes if len(codes) else np.zeros(1, dtype=np.uint8)), offsets

    def build_lm(self, codes, offsets, k, as_written=False, unseen="backoff", pseudocount=0.0, r_threshold=0.5, cut=0,
                 want_table=True, want_counts=False):
        """The RNA model of the transcripts in codes / offsets (lm.read_fasta), built on the device and left there as this
        context's LM, as load_lm would leave it (rd_lm_build; the contract is in include/radian_hip.h).  Returns (table [4^k,4] or
        None, stats); with want_counts stats["counts"] holds the order-k counts [4^k,4] uint32.  cut: input bytes per launch."""
        codes, offsets = self._records(codes, offsets)
        if unseen not in self.UNSEEN:
            raise ValueError(f"unseen must be one of {sorted(self.UNSEEN)}")
        big = 1 <= k <= 13
        table = np.empty((4 ** k, 4), dtype=np.float64) if want_table and big else None
        counts = np.empty((4 ** k, 4), dtype=np.uint32) if want_counts and big else None
        st = np.zeros(32, dtype=np.int64)
        self._check(self._L.rd_lm_build(self._h, _p(codes), _p(offsets), len(offsets) - 1, int(k), 1 if as_written else 0, self.UNSEEN[unseen],
                                        float(pseudocount), float(r_threshold), int(cut), _p(table), _p(counts), _p(st)))
        self.lm_k = k
        stats = {"windows": int(st[0]), "contexts": 4 ** k, "contexts_seen": int(st[1]), "gate_contexts": int(st[2]), "gate_windows": int(st[3]),
                 "absent_rows": int(st[4]), "uniform_rows": int(st[5]), "launches": int(st[6]),
                 "stage_us": {name: int(st[24 + i]) for i, name in enumerate(("staging", "upload", "count", "table", "download"))},
                 "rows_per_order": {j: int(st[8 + j]) for j in range(k, -1, -1) if st[8 + j]}}
        if counts is not None:
            stats["counts"] = counts
        return table, stats

    def score_lm(self, codes, offsets, as_written=False, r_threshold=0.5, cut=0):
        """Another set of transcripts against this context's LM (rd_lm_score): windows, how many have p > 0 / p = 0 / an absent
        context / an open gate, and the mean -ln p(next | context) over those with p > 0."""
        codes, offsets = self._records(codes, offsets)
        st = np.zeros(8, dtype=np.int64)
        total = ctypes.c_double(0.0)
        self._check(self._L.rd_lm_score(self._h, _p(codes), _p(offsets), len(offsets) - 1, 1 if as_written else 0, float(r_threshold), int(cut),
                                        _p(st), ctypes.byref(total)))
        n = int(st[1])
        return {"windows": int(st[0]), "scored": n, "zero": int(st[2]), "absent": int(st[3]), "gate_windows": int(st[4]),
                "nll_sum": total.value, "mean_nll": total.value / n if n else float("nan")}

    def load_lm_absent(self, k):
        """--context-len k with an RNA model whose keys have another length (rd_load_lm_absent): every lookup is the reference's KeyError."""
        self._check(self._L.rd_load_lm_absent(self._h, int(k)))
        self.lm_k = k

    def load_lm_hashed(self, table, table_order, context_len):
        """Synthetic LM for contexts longer than a dense table can index (rd_load_lm_hashed): table [4^table_order, 4],
        row = hash of the last `context_len` labels (<= 256)."""
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.shape != (4 ** table_order, 4):
            raise ValueError(f"LM table must be [4^{table_order},4], got {table.shape}")
        self._check(self._L.rd_load_lm_hashed(self._h, _p(table), int(table_order), int(context_len)))
        self.lm_k = context_len

    def set_logits(self, mode):
        """'f32' (default) or 'f16': storage of the softmax rows on the reads-level paths (rd_set_logits)."""
        self._check(self._L.rd_set_logits(self._h, {"f32": 0, "f16": 1}[mode] if isinstance(mode, str) else int(mode)))

    def set_trie_budget(self, nbytes):
        """workspace one beam-search launch may ask for (rd_set_trie_budget; 0 = the default 24 GiB): launches beyond it run as several
        runs of sequences sharing the workspace.  No effect on results -- tests set it small to exercise the cut."""
        self._check(self._L.rd_set_trie_budget(self._h, int(nbytes)))

    def set_conv_fuse(self, on):
        """block 0's first conv inside its second conv's kernel (default) or as a kernel of its own (rd_set_conv_fuse); same bits"""
        self._check(self._L.rd_set_conv_fuse(self._h, 1 if on else 0))

    def set_head_pack(self, on):
        """window heads of the chunk-mode reads paths as packed row classes without their zero-padding taps (default) or as head tiles
        (rd_set_head_pack); same bits"""
        self._check(self._L.rd_set_head_pack(self._h, 1 if on else 0))

    def head_pack_active(self):
        """whether the next chunk-mode forward packs its window heads (rd_head_pack_active): exact fp32, finite conv kernels, no -0.0 conv bias"""
        return bool(self._L.rd_head_pack_active(self._h))

    def head_pack_tiles(self):
        """packed window-head workgroup tiles the context's latest forward launched (rd_head_pack_tiles)"""
        return int(self._L.rd_head_pack_tiles(self._h))

    def set_conv_slab(self, on):
        """slab tiles of the exact-fp32 conv launches behind block 0 stage their input rows once per channel slice, or every tile once per
        tap (rd_set_conv_slab); same bits"""
        self._check(self._L.rd_set_conv_slab(self._h, 1 if on else 0))

    def conv_slab_active(self):
        """whether the next forward takes the slab path for its slab tiles (rd_conv_slab_active): the setting, exact fp32, 128-row tiles"""
        return bool(self._L.rd_conv_slab_active(self._h))

    def conv_slab_tiles(self):
        """slab workgroup tiles the context's latest forward launched, over all its conv launches (rd_conv_slab_tiles)"""
        return int(self._L.rd_conv_slab_tiles(self._h))

    def set_decode_form(self, form):
        """'auto' (default); 'waves' / 'lanes': launch shape for widths above 12; 'two' / 'one': widths up to 12 always / never as
        two sequences per wave; 'queue': every launch through the work-queue kernel with few resident workgroups (rd_set_decode_form)."""
        self._check(self._L.rd_set_decode_form(self._h, {"auto": 0, "waves": 1, "lanes": 2, "two": 3, "one": 4, "queue": 5}[form] if isinstance(form, str) else int(form)))

    def set_decode_partition(self, cus_per_xcd):
        """CUs per XCD reserved for the beam search of the global-mode reads pipeline (rd_set_decode_partition): -1 = by beam
        width (default), 0 = off."""
        self._check(self._L.rd_set_decode_partition(self._h, int(cus_per_xcd)))

    def set_decode_math(self, mode):
        """'glibc' (default: scores bit-identical to the reference's) or 'fast': arithmetic of the beam search's log / logaddexp
        (rd_set_decode_math)."""
        self._check(self._L.rd_set_decode_math(self._h, {"fast": 0, "glibc": 1}[mode] if isinstance(mode, str) else int(mode)))

    # ------------------------------------------------------------------ seams (host arrays)
    def forward(self, windows):
        """sig_model.predict (radian/basecall.py:91,93): [n,T] -> [n,T,5] float32."""
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        if windows.ndim != 2:
            raise ValueError("windows must be [n_windows, chunk_len]")
        n, T = windows.shape
        probs = np.empty((n, T, 5), dtype=np.float32)
        self._check(self._L.rd_forward(self._h, _p(windows), n, T, _p(probs)))
        return probs

    def assemble(self, probs, pad, step):
        """assemble_matrices after the pad trim (radian/basecall.py:96,100).  probs [nW,T,5] of one read."""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        nW, T, _ = probs.shape
        cap = (nW - 1) * step + T
        out = np.empty((max(cap, 1), 5), dtype=np.float64)
        n_rows = ctypes.c_int64(0)
        is64 = ctypes.c_int(0)
        self._check(self._L.rd_assemble(self._h, _p(probs), nW, T, int(pad), int(step), _p(out), out.shape[0],
                                        ctypes.byref(n_rows), ctypes.byref(is64)))
        out = out[: n_rows.value]
        return out if is64.value else out.astype(np.float32)

    def forward_reads(self, signals, chunk_len, step):
        """sig_model.predict over the windows of whole normalised reads (radian/basecall.py:83-93) through the streamed
        evaluation (rd_forward_reads): -> per read an array [nW, chunk_len, 5] float32 (rows the pad trim drops are zero)"""
        flat, off = self._pack_reads(signals)
        nws = [self.count_windows(off[r + 1] - off[r], chunk_len, step) for r in range(len(signals))]
        tot = int(sum(nws))
        out = np.zeros((tot, chunk_len, 5), dtype=np.float32)
        n = ctypes.c_int64(0)
        self._check(self._L.rd_forward_reads(self._h, _p(flat), _p(off), len(signals), int(chunk_len), int(step), _p(out), tot, ctypes.byref(n)))
        assert n.value == tot
        res, w = [], 0
        for k in nws:
            res.append(out[w:w + k])
            w += k
        return res

    def decode_batch(self, mats, seq_off, seq_len, beam_width, use_lm=False, s_threshold=0.0, r_threshold=0.0,
                     with_scores=False):
        """beam_search over a batch of sequences given as concatenated rows (radian/decode.py:100-212).
        Returns a list of uint8 label arrays (and the winners' log pr_total when with_scores)."""
        mats = np.ascontiguousarray(mats)
        if mats.dtype not in (np.float32, np.float64):
            raise TypeError("probabilities must be float32 or float64")
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
        n = int(seq_len.shape[0])
        label_off = np.zeros(n, dtype=np.int64)
        if n:
            label_off[1:] = np.cumsum(seq_len[:-1].astype(np.int64))
        labels = np.zeros(int(seq_len.astype(np.int64).sum()) + 1, dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        scores = np.zeros(n, dtype=np.float64) if with_scores else None
        self._check(self._L.rd_decode_batch(self._h, _p(mats), 1 if mats.dtype == np.float64 else 0, _p(seq_off), _p(seq_len), n,
                                            int(beam_width), 1 if use_lm else 0, float(s_threshold), float(r_threshold),
                                            _p(labels), _p(label_off), _p(lens), _p(scores)))
        out = [_labels_of(labels, label_off[i], lens[i]) for i in range(n)]
        return (out, scores) if with_scores else out

    def decode(self, mat, beam_width, use_lm=False, s_threshold=0.0, r_threshold=0.0):
        mat = np.ascontiguousarray(mat)
        return self.decode_batch(mat.reshape(-1, 5), [0], [mat.shape[0]], beam_width, use_lm, s_threshold, r_threshold)[0]

    # ------------------------------------------------------------------ fused paths
    def basecall_chunk(self, windows, valid_len, beam_width):
        """forward + LM-free per-window beam search (radian/basecall.py:86-96,110-121)."""
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        n, T = windows.shape
        valid_len = np.ascontiguousarray(valid_len, dtype=np.int32)
        labels = np.zeros((n, T), dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        self._check(self._L.rd_basecall_chunk(self._h, _p(windows), n, T, _p(valid_len), int(beam_width), _p(labels), _p(lens)))
        return [labels[i, : lens[i]].copy() for i in range(n)]

    def basecall_global(self, windows, read_win_off, pads, step, beam_width, use_lm, s_threshold=0.0, r_threshold=0.0):
        """forward + per-read assembly + one beam search per read (radian/basecall.py:86-109)."""
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        nW, T = windows.shape
        read_win_off = np.ascontiguousarray(read_win_off, dtype=np.int32)
        pads = np.ascontiguousarray(pads, dtype=np.int32)
        n_reads = pads.shape[0]
        caps = np.array([(read_win_off[r + 1] - read_win_off[r] - 1) * step + T - pads[r] for r in range(n_reads)], dtype=np.int64)
        caps = np.maximum(caps, 0)
        label_off = np.zeros(n_reads, dtype=np.int64)
        label_off[1:] = np.cumsum(caps[:-1])
        labels = np.zeros(int(caps.sum()) + 1, dtype=np.uint8)
        lens = np.zeros(n_reads, dtype=np.int32)
        self._check(self._L.rd_basecall_global(self._h, _p(windows), T, int(step), _p(read_win_off), _p(pads), n_reads,
                                               int(beam_width), 1 if use_lm else 0, float(s_threshold), float(r_threshold),
                                               _p(labels), _p(label_off), _p(lens)))
        return [_labels_of(labels, label_off[r], lens[r]) for r in range(n_reads)]

    # ------------------------------------------------------------------ reads-level fused paths
    def count_windows(self, n_samples, chunk_len, step):
        n = self._L.rd_count_windows(int(n_samples), int(chunk_len), int(step))
        if n < 0:
            raise ValueError("bad window geometry")
        return n

    @staticmethod
    def _pack_reads(signals):
        return _pack(signals, np.float32)

    def basecall_reads_chunk(self, signals, chunk_len, step, beam_width):
        """Chunk mode over whole (normalised) reads: returns, per read, the list of per-window label arrays
        (radian/basecall.py:83-121 without the host stitch).  Each time step is computed once (streamed forward)."""
        flat, off = self._pack_reads(signals)
        nw = [self.count_windows(off[r + 1] - off[r], chunk_len, step) for r in range(len(signals))]
        tot = int(sum(nw))
        labels = np.zeros((tot, chunk_len), dtype=np.uint8)
        lens = np.zeros(tot, dtype=np.int32)
        self._check(self._L.rd_basecall_reads_chunk(self._h, _p(flat), _p(off), len(signals), int(chunk_len), int(step),
                                                    int(beam_width), _p(labels), _p(lens)))
        return _window_labels(labels, lens, nw)

    def basecall_reads_global(self, signals, chunk_len, step, beam_width, use_lm, s_threshold=0.0, r_threshold=0.0):
        """Global mode over whole (normalised) reads (radian/basecall.py:83-109): one label array per read."""
        flat, off = self._pack_reads(signals)
        n = len(signals)
        labels = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        label_off = np.ascontiguousarray(off[:-1])
        self._check(self._L.rd_basecall_reads_global(self._h, _p(flat), _p(off), n, int(chunk_len), int(step), int(beam_width),
                                                     1 if use_lm else 0, float(s_threshold), float(r_threshold), _p(labels),
                                                     _p(label_off), _p(lens)))
        return [_labels_of(labels, off[r], lens[r]) for r in range(n)]

    # ------------------------------------------------------------------ raw int16 reads (normalisation on the device)
    STATUS_MESSAGES = {1: "MAD is zero, issue with signal.", 2: "Signal must not be empty to normalise"}  # preprocess.py:25-26,47-48

    @staticmethod
    def _pack_raw(raws):
        return _pack(raws, np.int16, pad=1)

    def normalise_reads(self, raws, outlier_clip):
        """float32(mad_normalise(raw, clip)) per read (radian/preprocess.py:24-49) + status per read (0 ok, 1 MAD zero, 2 empty)."""
        flat, off = self._pack_raw(raws)
        out = np.zeros(max(1, int(off[-1])), dtype=np.float32)
        status = np.zeros(len(raws), dtype=np.int32)
        self._check(self._L.rd_normalise_reads(self._h, _p(flat), _p(off), len(raws), int(outlier_clip), _p(out), _p(status)))
        return [out[off[r]:off[r + 1]].copy() for r in range(len(raws))], status

    def basecall_raw_chunk(self, raws, outlier_clip, chunk_len, step, beam_width):
        """raw int16 reads -> (per read list of per-window label arrays, status per read)."""
        flat, off = self._pack_raw(raws)
        nw = [self.count_windows(off[r + 1] - off[r], chunk_len, step) for r in range(len(raws))]
        tot = int(sum(nw))
        labels = np.zeros((tot, chunk_len), dtype=np.uint8)
        lens = np.zeros(tot, dtype=np.int32)
        status = np.zeros(len(raws), dtype=np.int32)
        self._check(self._L.rd_basecall_raw_chunk(self._h, _p(flat), _p(off), len(raws), int(outlier_clip), int(chunk_len), int(step),
                                                  int(beam_width), _p(labels), _p(lens), _p(status)))
        return _window_labels(labels, lens, nw), status

    def basecall_raw_global(self, raws, outlier_clip, chunk_len, step, beam_width, use_lm, s_threshold=0.0, r_threshold=0.0):
        flat, off = self._pack_raw(raws)
        n = len(raws)
        labels = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        label_off = np.ascontiguousarray(off[:-1])
        self._check(self._L.rd_basecall_raw_global(self._h, _p(flat), _p(off), n, int(outlier_clip), int(chunk_len), int(step),
                                                   int(beam_width), 1 if use_lm else 0, float(s_threshold), float(r_threshold),
                                                   _p(labels), _p(label_off), _p(lens), _p(status)))
        return [_labels_of(labels, off[r], lens[r]) for r in range(n)], status

    def basecall_raw_global_q(self, raws, outlier_clip, chunk_len, step, beam_width, use_lm, s_threshold=0.0, r_threshold=0.0,
                              budget_bytes=0, allow_too_large=False):
        """basecall_raw_global plus the forced alignment of every read's labels against the rows its beam search read
        (rd_basecall_raw_global_q): -> (labels per read, status per read, CtcAlignResult with one entry per read; the steps are
        sample indices into the read).  A read over the alignment budget raises, unless allow_too_large: it then comes back with
        status CTCALIGN_TOO_LARGE."""
        flat, off = self._pack_raw(raws)
        n = len(raws)
        cap = int(off[-1]) + 1
        labels = np.zeros(cap, dtype=np.uint8)
        qual = np.zeros(cap, dtype=np.uint8)
        first = np.full(cap, -1, dtype=np.int32)
        last = np.full(cap, -1, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        score = np.zeros(n, dtype=np.float64)
        ast = np.zeros(n, dtype=np.int32)
        label_off = np.ascontiguousarray(off[:-1])
        rc = self._L.rd_basecall_raw_global_q(self._h, _p(flat), _p(off), n, int(outlier_clip), int(chunk_len), int(step), int(beam_width),
                                              1 if use_lm else 0, float(s_threshold), float(r_threshold), _p(labels), _p(label_off), _p(lens),
                                              _p(status), int(budget_bytes), _p(qual), _p(first), _p(last), _p(score), _p(ast))
        if rc != 0 and not (allow_too_large and rc == -4 and (ast == CTCALIGN_TOO_LARGE).any()):
            self._check(rc)
        ln = [max(int(x), 0) for x in lens]
        res = CtcAlignResult([first[off[r]: off[r] + ln[r]].copy() for r in range(n)], [last[off[r]: off[r] + ln[r]].copy() for r in range(n)],
                             [qual[off[r]: off[r] + ln[r]].copy() for r in range(n)], score, ast)
        return [_labels_of(labels, off[r], lens[r]) for r in range(n)], status, res

    # ------------------------------------------------------------------ device-resident (bench)
    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._L.rd_dev_alloc(self._h, int(nbytes), ctypes.byref(p)))
        return p

    def mem_info(self):
        """(free, total) bytes of the context's device"""
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(self._L.rd_mem_info(self._h, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def dev_free(self, p):
        self._check(self._L.rd_dev_free(self._h, p))

    def h2d(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._check(self._L.rd_memcpy_h2d(self._h, d_ptr, _p(arr), arr.nbytes))

    def d2h(self, arr, d_ptr):
        self._check(self._L.rd_memcpy_d2h(self._h, _p(arr), d_ptr, arr.nbytes))

    def forward_resident(self, d_windows, n, T, d_probs=None):
        self._check(self._L.rd_forward_resident(self._h, d_windows, n, T, d_probs))

    def forward_reads_resident(self, d_signal, read_off, n_reads, chunk_len, step, decode_type="chunk", lane=0):
        """forward only over whole reads resident in HBM (rd_forward_reads_resident): asynchronous on `lane`; -> rows evaluated"""
        rows = ctypes.c_int64(0)
        self._check(self._L.rd_forward_reads_resident(self._h, d_signal, _p(read_off), int(n_reads), int(chunk_len), int(step),
                                                      {"chunk": 0, "global": 1}[decode_type], int(lane), ctypes.byref(rows)))
        return rows.value

    def basecall_chunk_resident(self, d_windows, n, T, valid_len, beam_width, labels, lens):
        self._check(self._L.rd_basecall_chunk_resident(self._h, d_windows, n, T, _p(valid_len), int(beam_width), _p(labels), _p(lens)))

    def decode_resident(self, d_probs, n, T, valid_len, beam_width, labels, lens):
        self._check(self._L.rd_decode_resident(self._h, d_probs, n, T, _p(valid_len), int(beam_width), _p(labels), _p(lens)))

    def pipe_submit(self, d_windows, n, T, valid_len, beam_width, labels, lens):
        """Pipelined chunk-mode batch of pre-cut windows resident in HBM (rd_pipe_submit); labels / lens are filled once
        pipe_progress reports the batch delivered (or at pipe_flush)."""
        self._check(self._L.rd_pipe_submit(self._h, d_windows, n, T, _p(valid_len), int(beam_width), _p(labels), _p(lens)))

    def pipe_submit_reads(self, d_signal, read_off, n_reads, chunk_len, step, beam_width, labels, lens):
        """Pipelined chunk-mode batch of whole normalised reads resident in HBM (rd_pipe_submit_reads); labels / lens are filled
        once pipe_progress reports the batch delivered (or at pipe_flush)."""
        self._check(self._L.rd_pipe_submit_reads(self._h, d_signal, _p(read_off), int(n_reads), int(chunk_len), int(step),
                                                 int(beam_width), _p(labels), _p(lens)))

    def basecall_reads_chunk_resident(self, d_signal, read_off, n_reads, chunk_len, step, beam_width, labels, lens):
        self._check(self._L.rd_basecall_reads_chunk_resident(self._h, d_signal, _p(read_off), int(n_reads), int(chunk_len),
                                                             int(step), int(beam_width), _p(labels), _p(lens)))

    def basecall_reads_global_resident(self, d_signal, read_off, n_reads, chunk_len, step, beam_width, use_lm, s_threshold,
                                       r_threshold, labels, label_off, lens):
        """Global mode over normalised reads resident in HBM (rd_basecall_reads_global_resident)."""
        self._check(self._L.rd_basecall_reads_global_resident(self._h, d_signal, _p(read_off), int(n_reads), int(chunk_len),
                                                              int(step), int(beam_width), 1 if use_lm else 0, float(s_threshold),
                                                              float(r_threshold), _p(labels), _p(label_off), _p(lens)))

    # ------------------------------------------------------------------ the context's pipeline (pipe_reads.hip)
    def pipe_submit_reads_global(self, d_signal, read_off, n_reads, chunk_len, step, beam_width, use_lm, s_threshold, r_threshold,
                                 labels, label_off, lens):
        """Pipelined global-mode batch of normalised reads resident in HBM (rd_pipe_submit_reads_global); labels / lens are
        filled once pipe_progress reports the batch delivered (or at pipe_flush)."""
        self._check(self._L.rd_pipe_submit_reads_global(self._h, d_signal, _p(read_off), int(n_reads), int(chunk_len), int(step),
                                                        int(beam_width), 1 if use_lm else 0, float(s_threshold), float(r_threshold),
                                                        _p(labels), _p(label_off), _p(lens)))

    def pipe_progress(self, wait_for=0):
        """Deliver finished groups of the pipeline; blocks until `wait_for` submits (counted over the context's
        life) are delivered when wait_for > 0.  -> number of submits delivered so far."""
        n = ctypes.c_int64(0)
        self._check(self._L.rd_pipe_progress(self._h, int(wait_for), ctypes.byref(n)))
        self._release_tickets(n.value)
        return n.value

    def _release_tickets(self, delivered):
        for seq in [q for q in self._tickets if q <= delivered]:
            del self._tickets[seq]

    def pipe_submit_raw(self, decode_type, raws, outlier_clip, chunk_len, step, beam_width, use_lm=False, s_threshold=0.0,
                        r_threshold=0.0):
        """Pipelined form of basecall_raw_global / basecall_raw_chunk: queue a batch of raw int16 reads and return a
        PipeTicket; ticket.result() gives what the unpipelined call returns once the batch is delivered."""
        flat, off = self._pack_raw(raws)
        n = len(raws)
        t = PipeTicket(self, decode_type, off, n)
        if decode_type == "global":
            t.labels = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
            t.lens = np.zeros(n, dtype=np.int32)
            t.label_off = np.ascontiguousarray(off[:-1])
            self._check(self._L.rd_pipe_submit_raw_global(self._h, _p(flat), _p(off), n, int(outlier_clip), int(chunk_len), int(step),
                                                          int(beam_width), 1 if use_lm else 0, float(s_threshold), float(r_threshold),
                                                          _p(t.labels), _p(t.label_off), _p(t.lens), _p(t.status)))
        else:
            t.nw = [self.count_windows(off[r + 1] - off[r], chunk_len, step) for r in range(n)]
            tot = int(sum(t.nw))
            t.labels = np.zeros((tot, chunk_len), dtype=np.uint8)
            t.lens = np.zeros(tot, dtype=np.int32)
            self._check(self._L.rd_pipe_submit_raw_chunk(self._h, _p(flat), _p(off), n, int(outlier_clip), int(chunk_len), int(step),
                                                         int(beam_width), _p(t.labels), _p(t.lens), _p(t.status)))
        t.seq = self.pipe_submitted()
        self._tickets[t.seq] = t
        return t

    def pipe_submitted(self):
        """batches submitted to the pipeline so far = the pipe_progress count at which the latest one is delivered"""
        n = ctypes.c_int64(0)
        self._check(self._L.rd_pipe_submitted(self._h, ctypes.byref(n)))
        return n.value

    def pipe_stats(self):
        """counters of the pipeline (rd_pipe_stats)"""
        v = (ctypes.c_int64 * 5)()
        self._check(self._L.rd_pipe_stats(self._h, v, 5))
        return dict(zip(("submitted", "delivered", "launches", "queue_launches", "limit_closes"), (int(x) for x in v)))

    def pipe_policy(self, beam_width, on_partition, use_lm=False):
        """what the context has measured for its global-mode group policy (rd_pipe_policy_read): ns per forward row, us per time
        step of a group's longest chain (0.0: not measured yet) and the rule in force, forward rows per chain step.  on_partition:
        1..3 = waves per SIMD of the decode partition, 0 = the whole chip"""
        ns, us, rows = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._L.rd_pipe_policy_read(self._h, int(beam_width), int(on_partition), 1 if use_lm else 0, ctypes.byref(ns),
                                                ctypes.byref(us), ctypes.byref(rows)))
        return {"ns_per_row": ns.value, "us_per_step": us.value, "rows_per_step": rows.value}

    def pipe_config(self, group_batches):
        self._check(self._L.rd_pipe_config(self._h, int(group_batches)))

    def pipe_set_lanes(self, lanes):
        """forward streams the submitted batches rotate over (1..4, default 2)"""
        self._check(self._L.rd_pipe_set_lanes(self._h, int(lanes)))

    def pipe_flush(self):
        self._check(self._L.rd_pipe_flush(self._h))
        self._release_tickets(self.pipe_submitted())

    def timer_enable(self, which, max_launches):
        self._check(self._L.rd_timer_enable(self._h, which, max_launches))

    def timer_read(self, which):
        ms = ctypes.c_double()
        n = ctypes.c_int()
        fl = ctypes.c_double()
        by = ctypes.c_double()
        self._check(self._L.rd_timer_read(self._h, which, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)))
        return {"total_ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    def timer_read_launches(self, which, cap=4096):
        """the recorded launches one by one (rd_timer_read_launches): (ms float32[n], flops float64[n], tag int32[n])"""
        ms = np.zeros(cap, dtype=np.float32)
        fl = np.zeros(cap, dtype=np.float64)
        tag = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_int()
        self._check(self._L.rd_timer_read_launches(self._h, which, int(cap), _p(ms), _p(fl), _p(tag), ctypes.byref(n)))
        return ms[: n.value], fl[: n.value], tag[: n.value]

    # ------------------------------------------------------------------ multi-GPU start-up
    def rccl_probe(self):
        """librccl loads in this process (no communicator, no bootstrap thread)."""
        self._check(self._L.rd_rccl_probe())

    def rccl_unique_id(self):
        buf = (ctypes.c_uint8 * 128)()
        self._check(self._L.rd_rccl_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return bytes(buf)

    def rccl_init(self, rank, nranks, uid):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self._L.rd_rccl_init(self._h, rank, nranks, ctypes.cast(buf, ctypes.c_void_p)))

    def rccl_finalize(self):
        self._check(self._L.rd_rccl_finalize(self._h))

    def clone_artifacts_from(self, src):
        """Take the loaded weights (every packing) and LM table of another Backend of this process by a device copy
        (rd_clone_artifacts): the receiver's code of the multi-GPU broadcast, without parsing / repacking again."""
        self._check(self._L.rd_clone_artifacts(self._h, src._h))

    def rccl_bcast_model(self, root=0):
        self._check(self._L.rd_rccl_bcast_model(self._h, root))

    def rccl_allreduce_max(self, values):
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._L.rd_rccl_allreduce_max(self._h, _p(a), a.size))
        return a

    def rccl_barrier(self):
        self._check(self._L.rd_rccl_barrier(self._h))

    def rccl_comm_count(self):
        """ranks in the communicator as RCCL reports them (ncclCommCount)"""
        n = ctypes.c_int(0)
        self._check(self._L.rd_rccl_comm_count(self._h, ctypes.byref(n)))
        return n.value

    # ------------------------------------------------------------------ read-accuracy evaluation (radian/align.py)
    def align(self, refs, reads, scores=ALIGN_SCORES, budget_bytes=0, with_ops=False, allow_too_large=False):
        """Global affine-gap alignment of reads[p] against refs[p] (str or bytes, compared byte by byte) and analyse_alignment's
        clip + counts, on the GPU (rd_align_batch).  scores: match, mismatch, gap_open, gap_extend with gap_open <= gap_extend (the
        library refuses open > extend: the recurrence would reopen adjacent gaps).  budget_bytes: device workspace per batch,
        0 = a quarter of free memory.
        A pair that does not fit the budget raises, unless allow_too_large: it then comes back with status ALIGN_TOO_LARGE."""
        if len(refs) != len(reads):
            raise ValueError(f"{len(refs)} refs for {len(reads)} reads")
        n = len(refs)
        rbuf, roff = _concat(refs)
        qbuf, qoff = _concat(reads)
        score = np.zeros(n, dtype=np.int32)
        counts = np.zeros((n, 4), dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        ops = ops_off = ops_len = None
        if with_ops:
            ops_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum((roff[1:] - roff[:-1]) + (qoff[1:] - qoff[:-1]), out=ops_off[1:])
            ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.uint8)
            ops_len = np.zeros(n, dtype=np.int32)
        m, x, go, ge = (int(v) for v in scores)
        rc = self._L.rd_align_batch(self._h, _p(rbuf), _p(roff), _p(qbuf), _p(qoff), n, m, x, go, ge, int(budget_bytes), _p(score),
                                    _p(counts), _p(status), _p(ops), _p(ops_off), _p(ops_len))
        if rc != 0 and not (allow_too_large and rc == -4 and (status == ALIGN_TOO_LARGE).any()):
            self._check(rc)
        ops_list = None
        if with_ops:
            ops_list = [ops[ops_off[p]: ops_off[p] + ops_len[p]].tobytes() for p in range(n)]
        return AlignResult(score, counts, status, ops_list)

    # ------------------------------------------------------------------ pileup
    def pileup_open(self, n_sites):
        """Allocate and zero the context's pileup tables for n_sites sites (rd_pileup_open); a second open starts again from zero."""
        self._check(self._L.rd_pileup_open(self._h, int(n_sites)))

    def pileup_close(self):
        self._check(self._L.rd_pileup_close(self._h))

    def pileup_add(self, refs, reads, site0, scores=ALIGN_SCORES, budget_bytes=0, with_ops=False, allow_too_large=False):
        """Align reads[p] against the span refs[p] exactly as Backend.align does and add the alignment's columns to the open pileup, the
        span's first base being site site0[p] (rd_pileup_add).  A pair over the budget raises, unless allow_too_large: status
        PILEUP_TOO_LARGE, nothing added for it."""
        n, rbuf, roff, qbuf, qoff, s0, out, _, _ = _pileup_args(refs, reads, site0)
        ops = ops_off = ops_len = None
        if with_ops:
            ops_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum((roff[1:] - roff[:-1]) + (qoff[1:] - qoff[:-1]), out=ops_off[1:])
            ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.uint8)
            ops_len = np.zeros(max(n, 1), dtype=np.int32)
        m, x, go, ge = (int(v) for v in scores)
        rc = self._L.rd_pileup_add(self._h, _p(rbuf), _p(roff), _p(qbuf), _p(qoff), n, _p(s0), m, x, go, ge, int(budget_bytes), _p(out),
                                   _p(ops), _p(ops_off), _p(ops_len))
        if rc != 0 and not (allow_too_large and rc == -4 and (out[:n, 0] == PILEUP_TOO_LARGE).any()):
            self._check(rc)
        ops_list = [ops[ops_off[p]: ops_off[p] + ops_len[p]].tobytes() for p in range(n)] if with_ops else None
        return PileupPairs(out[:n], ops_list)

    def pileup_add_ops(self, ops, refs, reads, site0):
        """Add alignments the caller already has (ops[p]: bytes of M / X / D / I that consume refs[p] and reads[p] exactly) to the open
        pileup; no alignment runs (rd_pileup_add_ops)."""
        n, rbuf, roff, qbuf, qoff, s0, out, obuf, ooff = _pileup_args(refs, reads, site0, ops)
        self._check(self._L.rd_pileup_add_ops(self._h, _p(obuf), _p(ooff), _p(rbuf), _p(roff), _p(qbuf), _p(qoff), n, _p(s0), _p(out)))
        return PileupPairs(out[:n])

    def pileup_read(self, min_depth=1, capacity=None):
        """The sites at depth >= min_depth, in site order, and the profile (rd_pileup_read).  capacity None: asked for first."""
        profile = np.zeros(PILEUP_PROFILE_LEN, dtype=np.uint64)
        n_out = ctypes.c_int64(0)
        if capacity is None:
            rc = self._L.rd_pileup_read(self._h, int(min_depth), 0, None, None, _p(profile), ctypes.byref(n_out))
            if rc != 0 and n_out.value == 0:
                self._check(rc)
            capacity = n_out.value
        site = np.zeros(max(int(capacity), 1), dtype=np.uint32)
        counts = np.zeros((max(int(capacity), 1), 8), dtype=np.uint32)
        self._check(self._L.rd_pileup_read(self._h, int(min_depth), int(capacity), _p(site), _p(counts), _p(profile), ctypes.byref(n_out)))
        return PileupTable(site[:n_out.value], counts[:n_out.value], profile)

    # ------------------------------------------------------------------ forced CTC alignment
    def ctc_align(self, mats, seq_off, seq_len, labels, budget_bytes=0, allow_too_large=False):
        """Forced (Viterbi) CTC alignment of labels[i] (codes 0..3) against rows seq_off[i] .. + seq_len[i] of mats ([rows,5] float32 or
        float64), on the GPU (rd_ctc_align_batch; the contract is in include/radian_hip.h).  budget_bytes: device workspace per launch,
        0 = a quarter of free memory.  A sequence that does not fit it raises, unless allow_too_large: status CTCALIGN_TOO_LARGE."""
        mats = np.ascontiguousarray(mats)
        if mats.dtype not in (np.float32, np.float64):
            raise TypeError("probabilities must be float32 or float64")
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
        n = int(seq_len.shape[0])
        if len(labels) != n:
            raise ValueError(f"{len(labels)} label sequences for {n} sequences")
        if n and int((seq_off + seq_len).max()) > mats.reshape(-1, 5).shape[0]:
            raise ValueError("a sequence reaches past the rows given")
        labs = [np.ascontiguousarray(x, dtype=np.uint8).ravel() for x in labels]
        label_len = np.array([x.shape[0] for x in labs], dtype=np.int32)
        label_off = np.zeros(n, dtype=np.int64)
        if n:
            label_off[1:] = np.cumsum(label_len[:-1].astype(np.int64))
        tot = int(label_len.astype(np.int64).sum())
        lbuf = np.zeros(tot + 1, dtype=np.uint8)
        if tot:
            lbuf[:tot] = np.concatenate(labs)
        first = np.full(tot + 1, -1, dtype=np.int32)
        last = np.full(tot + 1, -1, dtype=np.int32)
        qual = np.zeros(tot + 1, dtype=np.uint8)
        score = np.zeros(n, dtype=np.float64)
        status = np.zeros(n, dtype=np.int32)
        rc = self._L.rd_ctc_align_batch(self._h, _p(mats), 1 if mats.dtype == np.float64 else 0, _p(seq_off), _p(seq_len), n, _p(lbuf),
                                        _p(label_off), _p(label_len), int(budget_bytes), _p(first), _p(last), _p(qual), _p(score), _p(status))
        if rc != 0 and not (allow_too_large and rc == -4 and (status == CTCALIGN_TOO_LARGE).any()):
            self._check(rc)
        cut = [(int(label_off[i]), int(label_off[i] + label_len[i])) for i in range(n)]
        return CtcAlignResult([first[a:b].copy() for a, b in cut], [last[a:b].copy() for a, b in cut], [qual[a:b].copy() for a, b in cut],
                              score, status)

    # ------------------------------------------------------------------ poly(A) tail estimation
    def polya_segment(self, raws, params, budget_bytes=0, allow_too_large=False):
        """The longest flat segment of every read's raw samples (rd_polya_segment, on the GPU): raws -- one int16 array per read; params --
        a PolyaParams.  budget_bytes: device workspace per launch, 0 = a quarter of free memory.  A read that does not fit it raises,
        unless allow_too_large: status POLYA_TOO_LARGE.  -> PolyaResult."""
        flat, off = self._pack_raw(raws)
        res = PolyaResult(len(raws))
        rc = self._L.rd_polya_segment(self._h, _p(flat), _p(off), len(raws), *params.args(), int(budget_bytes), *res._bufs())
        if rc != 0 and not (allow_too_large and rc == -4 and (res.status == POLYA_TOO_LARGE).any()):
            self._check(rc)
        return res._cut(len(raws))

    polya_segment_host = staticmethod(polya_segment_host)

    def polya_diag_windows(self, raws, params):
        """rd_polya_diag_windows (tests): the scale and window stages alone.  -> (m2, d4 int32 [reads], thr uint64 [reads], per read the
        int32 S, int64 Q and uint8 flag of its windows)"""
        flat, off = self._pack_raw(raws)
        n = len(raws)
        nw = [int(off[r + 1] - off[r]) // params.win for r in range(n)]
        woff = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
        tot = int(woff[-1])
        m2, d4, thr = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.uint64)
        S, Q, F = np.zeros(tot + 1, np.int32), np.zeros(tot + 1, np.int64), np.zeros(tot + 1, np.uint8)
        self._check(self._L.rd_polya_diag_windows(self._h, _p(flat), _p(off), n, params.win, params.flat_q, params.use_level, params.lo_q,
                                                  params.hi_q, _p(m2), _p(d4), _p(thr), _p(S), _p(Q), _p(F)))
        cut = [(int(woff[r]), int(woff[r + 1])) for r in range(n)]
        return m2[:n], d4[:n], thr[:n], [(S[a:b].copy(), Q[a:b].copy(), F[a:b].copy()) for a, b in cut]

    # ------------------------------------------------------------------ event detection
    def segment(self, raws, params, scale_windows=None, budget_bytes=0, allow_too_large=False):
        """Every read's raw samples cut into events (rd_segment, on the GPU): raws -- one int16 array per read; params -- a SegmentParams;
        scale_windows -- per read (lo, hi) in the read's samples, whose scale comes back as m2 / d4.  budget_bytes: device workspace per
        launch, 0 = a quarter of free memory.  A read that does not fit it raises, unless allow_too_large: status SEGMENT_TOO_LARGE.
        -> SegmentResult."""
        rc, res = _segment_call(lambda *a: self._L.rd_segment(self._h, *a), raws, params, scale_windows, (int(budget_bytes),))
        if rc != 0 and not (allow_too_large and rc == -4 and (res.status == SEGMENT_TOO_LARGE).any()):
            self._check(rc)
        return res

    segment_host = staticmethod(segment_host)

    def segment_diag_tstat(self, raws, params):
        """rd_segment_diag_tstat (tests): the first stage alone.  -> per read (N uint64 [2][T], D uint64 [2][T], peak bits uint8 [T])"""
        flat, off = self._pack_raw(raws)
        n, tot = len(raws), int(off[-1])
        F = np.zeros(tot + 1, np.uint8)
        Nc, Dc =np.zeros(2 * tot + 1, np.uint64), np.zeros(2 * tot + 1, np.uint64)
        self._check(self._L.rd_segment_diag_tstat(self._h, _p(flat), _p(off), n, *params.args(), _p(Nc), _p(Dc), _p(F)))
        N, D = Nc[:2 * tot].reshape(2, tot), Dc[:2 * tot].reshape(2, tot)
        return [(N[:, int(off[r]):int(off[r + 1])].copy(), D[:, int(off[r]):int(off[r + 1])].copy(), F[int(off[r]):int(off[r + 1])].copy()) for r in range(n)]

    # ------------------------------------------------------------------ two-sample site comparison
    def site_compare(self, site, cond, value, n_sites, budget_bytes=0, capacity=None, allow_too_large=False):
        """Both samples' events side by side, site by site (rd_site_compare, on the GPU): site uint32 (< n_sites), cond uint8 (0 / 1), value
        int16, one entry per event.  capacity: entries the outputs hold (default: the number of distinct sites).  budget_bytes: device
        workspace per launch, 0 = a quarter of free memory.  A site that does not fit it raises, unless allow_too_large: status
        SITE_TOO_LARGE.  -> SiteResult."""
        site, cond, value, capacity = _site_args(site, cond, value, capacity)
        res, n_out = SiteResult(capacity), ctypes.c_int64(0)
        rc = self._L.rd_site_compare(self._h, _p(site), _p(cond), _p(value), site.shape[0], int(n_sites), int(budget_bytes), capacity, *res._bufs(),
                                     ctypes.byref(n_out))
        if rc != 0 and not (allow_too_large and rc == -4 and (res.status[:n_out.value] == SITE_TOO_LARGE).any()):
            self._check(rc)
        return res._cut(n_out.value)

    site_compare_host = staticmethod(site_compare_host)

    # ------------------------------------------------------------------ exact two-cluster split per site
    def site_split(self, site, cond, value, n_sites, min_frac_q16=0, budget_bytes=0, capacity=None, allow_too_large=False):
        """The threshold on every site's pooled values that maximises the between-cluster score, among cuts that leave both clusters at
        least min_frac_q16 / 65536 of the events (rd_site_split, on the GPU).  Arguments as site_compare.  -> SplitResult."""
        site, cond, value, capacity = _site_args(site, cond, value, capacity)
        res, n_out = SplitResult(capacity), ctypes.c_int64(0)
        rc = self._L.rd_site_split(self._h, _p(site), _p(cond), _p(value), site.shape[0], int(n_sites), int(budget_bytes), capacity,
                                   int(min_frac_q16), *res._bufs(), ctypes.byref(n_out))
        if rc != 0 and not (allow_too_large and rc == -4 and (res.status[:n_out.value] == SITE_TOO_LARGE).any()):
            self._check(rc)
        return res._cut(n_out.value)

    site_split_host = staticmethod(site_split_host)
    site_split_workspace_bytes = staticmethod(site_split_workspace_bytes)

    def site_diag_segments(self, site, cond, value, n_sites):
        """rd_site_diag_segments (tests): the pack, sort and segment stages alone.  -> (sorted keys uint64 [events], segments int64 [sites, 4]:
        site, start, split, end)"""
        site, cond, value, capacity = _site_args(site, cond, value, None)
        keys, segs, n_seg = np.zeros(site.shape[0] + 1, np.uint64), np.zeros((capacity + 1, 4), np.int64), ctypes.c_int64(0)
        self._check(self._L.rd_site_diag_segments(self._h, _p(site), _p(cond), _p(value), site.shape[0], int(n_sites), capacity, _p(keys), _p(segs),
                                                  ctypes.byref(n_seg)))
        return keys[:site.shape[0]], segs[:n_seg.value]

    # ------------------------------------------------------------------ signal simulation
    def sim_lengths(self, seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift=None, dwell_scale=None,
                    budget_bytes=0):
        """The number of samples every read comes to (rd_sim_lengths, on the GPU): seqs -- one uint8 code array per read, in pore order;
        model -- a SimModel; the per-read integers as arrays or scalars; keys uint32 [reads, 2]; level_shift / dwell_scale -- None or one
        array per read with an entry per base.  -> int64 [reads]"""
        keep, args, off = _sim_args(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
        out = np.zeros(len(seqs) + 1, dtype=np.int64)
        self._check(self._L.rd_sim_lengths(self._h, *args, int(budget_bytes), _p(out)))
        return out[:len(seqs)]

    def sim_signal(self, seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift=None, dwell_scale=None,
                   n_samples=None, budget_bytes=0, allow_too_large=False):
        """The raw samples of every read and every base's first sample (rd_sim_signal, on the GPU); arguments as sim_lengths.  n_samples:
        the reads' lengths when the caller has them (sim_lengths otherwise).  budget_bytes: device workspace per launch, 0 = a quarter of
        free memory.  A read that does not fit it raises, unless allow_too_large: status SIM_TOO_LARGE.  -> SimResult."""
        n = len(seqs)
        if n_samples is None:
            n_samples = self.sim_lengths(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
        keep, args, off = _sim_args(seqs, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, keys, level_shift, dwell_scale)
        raw_off = np.zeros(n + 1, dtype=np.int64)
        raw_off[1:] = np.cumsum(np.asarray(n_samples, dtype=np.int64))
        raw, bf, status = np.zeros(int(raw_off[-1]) + 1, np.int16), np.zeros(int(off[-1]) + 1, np.int32), np.zeros(n + 1, np.int32)
        rc = self._L.rd_sim_signal(self._h, *args, _p(raw_off), int(budget_bytes), _p(raw), _p(bf), _p(status))
        if rc != 0 and not (allow_too_large and rc == -4 and (status[:n] == SIM_TOO_LARGE).any()):
            self._check(rc)
        return _sim_result(raw, raw_off, bf, off, status[:n], n)

    sim_lengths_host = staticmethod(sim_lengths_host)
    sim_signal_host = staticmethod(sim_signal_host)

    # ------------------------------------------------------------------ eventalign against a pore model
    def eventalign(self, raws, seqs, model, t_lo=None, t_hi=None, m2=None, d4=None, budget_bytes=0, allow_too_large=False):
        """The Viterbi path of every read's bases through its samples under a k-mer pore model (rd_eventalign, on the GPU): raws -- one
        int16 array per read; seqs -- one uint8 code array per read, in pore order; model -- an EvalModel; t_lo / t_hi -- the window of
        every read (default: the whole read); m2 / d4 -- the scale of every read (d4 0, the default: the window's own).  budget_bytes:
        device workspace per launch, 0 = a quarter of free memory.  A read that does not fit it raises, unless allow_too_large: status
        EVAL_TOO_LARGE.  -> EvalResult."""
        keep, head, outs, cut = _eval_args(raws, seqs, model, t_lo, t_hi, m2, d4)
        rc = self._L.rd_eventalign(self._h, *head, int(budget_bytes), *[_p(b) for b in outs])
        if rc != 0 and not (allow_too_large and rc == -4 and (outs[0][:len(raws)] == EVAL_TOO_LARGE).any()):
            self._check(rc)
        return _eval_result(outs, cut, len(raws))

    eventalign_host = staticmethod(eventalign_host)

    def eventalign_events(self, events, n_samples, seqs, model, m2, d4, sample_off=None, skip_pen=96, budget_bytes=0, allow_too_large=False):
        """The Viterbi path of every read's bases through its EVENTS, each weighted by its sample count, with skips of one base
        (rd_eventalign_events, on the GPU): events -- per read the dict of arrays a SegmentResult holds (start, sum,
        sumsq, min, max); n_samples -- the length of the window the events cut; seqs, model -- as eventalign; m2 / d4 -- the scale of every
        read, always given; sample_off -- added to every sample index reported; skip_pen -- -1: no skips, otherwise 0..256 in 1/32 nat.
        budget_bytes and allow_too_large as eventalign.  -> EvalRowsResult."""
        keep, head, outs, cut = _eval_rows_args(events, n_samples, seqs, model, m2, d4, sample_off, skip_pen)
        rc = self._L.rd_eventalign_events(self._h, *head, int(budget_bytes), *[_p(b) for b in outs])
        if rc != 0 and not (allow_too_large and rc == -4 and (outs[0][:len(events)] == EVAL_TOO_LARGE).any()):
            self._check(rc)
        return _eval_rows_result(keep, outs, cut, len(events))

    eventalign_events_host = staticmethod(eventalign_events_host)
    eventalign_events_workspace_bytes = staticmethod(eventalign_events_workspace_bytes)

    def eventalign_banded(self, raws, seqs, guides, model, t_lo=None, t_hi=None, m2=None, d4=None, budget_bytes=0, allow_too_large=False):
        """eventalign over a window of EVAL_BAND_W states that slides with a guide (rd_eventalign_banded, on the GPU):
        guides -- per read one int32 per base, the read sample the base is expected to start at, non-decreasing (what eventalign_events
        returns as events[r]["start"]); everything else as eventalign.  Where eventalign's own path stays inside the window the result is
        eventalign's; a read whose path the window lost has status EVAL_OFF_BAND.  -> EvalBandedResult."""
        keep, head, outs, cut = _eval_banded_args(raws, seqs, guides, model, t_lo, t_hi, m2, d4)
        rc = self._L.rd_eventalign_banded(self._h, *head, int(budget_bytes), *[_p(b) for b in outs])
        if rc != 0 and not (allow_too_large and rc == -4 and (outs[0][:len(raws)] == EVAL_TOO_LARGE).any()):
            self._check(rc)
        return _eval_banded_result(outs, cut, len(raws))

    eventalign_banded_host = staticmethod(eventalign_banded_host)
    eventalign_banded_workspace_bytes = staticmethod(eventalign_banded_workspace_bytes)

    # ------------------------------------------------------------------ per-read modification calls
    def modcall(self, raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts, flank=6, budget_bytes=0, allow_too_large=False):
        """Per (read, site) job the likelihood of the rows round the site under the canonical states and under the job's own (rd_modcall,
        on the GPU): raws, seqs, model -- as eventalign (the background takes no part); m2 / d4 -- the scale of every read, always given;
        firsts / lasts -- per read one int32 per base, the read samples the base's rows start and end at (an EvalResult's first_step and
        last_step, or events[r]["start"] and events[r]["end"] - 1; -1: no rows); job_read, alt_first -- per job its read and the first
        base whose state is replaced; alts -- per job (lvl, w, bias) of the 1..9 replacing entries; flank -- bases either side, 0..27.
        budget_bytes and allow_too_large as eventalign (status MC_TOO_LARGE).  -> ModcallResult."""
        keep, head, outs = _modcall_args(raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts, flank)
        rc = self._L.rd_modcall(self._h, *head, int(budget_bytes), *[_p(b) for b in outs])
        if rc != 0 and not (allow_too_large and rc == -4 and (outs[0][:len(job_read)] == MC_TOO_LARGE).any()):
            self._check(rc)
        return ModcallResult(*[b[:len(job_read)] for b in outs])

    modcall_host = staticmethod(modcall_host)
    modcall_workspace_bytes = staticmethod(modcall_workspace_bytes)

    # ------------------------------------------------------------------ signal against a panel of targets
    def sigmap(self, raw, targets, model, q_lo, q_hi, sc_lo=None, sc_hi=None, m2=None, d4=None, s_lo=None, s_hi=None, n_best=1,
               budget_bytes=0, allow_too_large=False):
        """The targets of a panel that every query's samples fit best under a k-mer pore model, with a free start and end in the target
        (rd_sigmap, on the GPU): raw -- one int16 array, every index below is absolute into it; targets -- one uint8 code array per target
        in pore order, or a SigmapPanel (sigmap_panel packs one once); model -- an EvalModel (its background is not used); q_lo / q_hi -- the rows of every query;
        sc_lo / sc_hi -- its scale window (default: the query's); m2 / d4 -- its scale (d4 0, the default: the scale window's own);
        s_lo / s_hi -- its range of global states (default: the whole panel); n_best 1..8.  budget_bytes: device workspace per launch,
        0 = a quarter of free memory.  A query that does not fit it raises, unless allow_too_large: status SIGMAP_TOO_LARGE.
        -> SigmapResult."""
        keep, head, outs = _sigmap_args(raw, targets, model, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best)
        rc = self._L.rd_sigmap(self._h, *head, int(budget_bytes), *[_p(b) for b in outs])
        if rc != 0 and not (allow_too_large and rc == -4 and (outs[0][:head[2]] == SIGMAP_TOO_LARGE).any()):
            self._check(rc)
        return _sigmap_result(outs, head[2], int(n_best))

    sigmap_host = staticmethod(sigmap_host)

    # ------------------------------------------------------------------ signal-to-reference alignment
    def event_stats(self, raws, aln):
        """The event table of an alignment whose rows are the reads' samples (rd_event_stats, on the GPU): raws -- one int16 array per read;
        aln -- a CtcAlignResult with one entry per read (first_step / last_step as sample indices, status).  -> EventsResult."""
        flat, off, n, fbuf, lbuf, label_off, label_len, status, tot, cut = _event_args(raws, aln)
        bufs = _event_buffers(tot)
        self._check(self._L.rd_event_stats(self._h, _p(flat), _p(off), n, _p(fbuf), _p(lbuf), _p(label_off), _p(label_len), _p(status),
                                           *[_p(b) for b in bufs]))
        return _events_of(bufs, cut)

    event_stats_host = staticmethod(event_stats_host)

    def resquiggle_raw(self, raws, ref_labels, outlier_clip, chunk_len, step, budget_bytes=0, allow_too_large=False):
        """Signal-to-reference alignment (rd_resquiggle_raw): raw int16 reads and, per read, the labels to put on its signal (codes 0..3 in
        decode order) -> (CtcAlignResult, EventsResult, read status), one entry per read; steps and events are sample indices into the read.
        No beam search.  A read over the alignment budget raises, unless allow_too_large: status CTCALIGN_TOO_LARGE."""
        flat, off = self._pack_raw(raws)
        n = len(raws)
        if len(ref_labels) != n:
            raise ValueError(f"{len(ref_labels)} label sequences for {n} reads")
        labs = [np.ascontiguousarray(x, dtype=np.uint8).ravel() for x in ref_labels]
        ref_len = np.array([x.shape[0] for x in labs], dtype=np.int32)
        ref_off = np.zeros(n, dtype=np.int64)
        if n:
            ref_off[1:] = np.cumsum(ref_len[:-1].astype(np.int64))
        tot = int(ref_len.astype(np.int64).sum())
        lbuf = np.zeros(tot + 1, dtype=np.uint8)
        if tot:
            lbuf[:tot] = np.concatenate(labs)
        first = np.full(tot + 1, -1, dtype=np.int32)
        last = np.full(tot + 1, -1, dtype=np.int32)
        qual = np.zeros(tot + 1, dtype=np.uint8)
        score = np.zeros(n, dtype=np.float64)
        ast = np.zeros(n, dtype=np.int32)
        rst = np.zeros(n, dtype=np.int32)
        bufs = _event_buffers(tot)
        rc = self._L.rd_resquiggle_raw(self._h, _p(flat), _p(off), n, int(outlier_clip), int(chunk_len), int(step), _p(lbuf), _p(ref_off),
                                       _p(ref_len), int(budget_bytes), _p(first), _p(last), _p(qual), _p(score), _p(ast), _p(rst),
                                       *[_p(b) for b in bufs])
        if rc != 0 and not (allow_too_large and rc == -4 and (ast == CTCALIGN_TOO_LARGE).any()):
            self._check(rc)
        cut = [(int(ref_off[i]), int(ref_off[i] + ref_len[i])) for i in range(n)]
        aln = CtcAlignResult([first[a:b].copy() for a, b in cut], [last[a:b].copy() for a, b in cut], [qual[a:b].copy() for a, b in cut],
                             score, ast)
        return aln, _events_of(bufs, cut), rst

    # ------------------------------------------------------------------ label windows: fitting alignment (radian_amd/label_build.py)
    def fit_batch(self, refs, queries, query_ref, scores=ALIGN_SCORES, budget_bytes=0, allow_too_large=False):
        """Fit queries[p] (codes 0..3) into refs[query_ref[p]] (codes 0..4, 4 matching nothing): the whole query aligned, the
        reference free before and after the span, on the GPU (rd_fit_batch).  budget_bytes: device buffer per batch, 0 = a quarter of
        free memory.  A query that does not fit the budget raises, unless allow_too_large: it then comes back with FIT_TOO_LARGE."""
        if len(query_ref) != len(queries):
            raise ValueError(f"{len(query_ref)} reference indices for {len(queries)} queries")
        rbuf, roff = _concat_codes(refs)
        qbuf, qoff = _concat_codes(queries)
        return self.fit_batch_flat(rbuf, roff, qbuf, qoff, query_ref, scores, budget_bytes, allow_too_large)

    def fit_batch_flat(self, rbuf, roff, qbuf, qoff, query_ref, scores=ALIGN_SCORES, budget_bytes=0, allow_too_large=False):
        """fit_batch on the C ABI's own layout: codes back to back (uint8) and int64 offsets with count + 1 entries"""
        roff, qoff = np.ascontiguousarray(roff, dtype=np.int64), np.ascontiguousarray(qoff, dtype=np.int64)
        rbuf, qbuf = np.ascontiguousarray(rbuf, dtype=np.uint8), np.ascontiguousarray(qbuf, dtype=np.uint8)
        n = len(qoff) - 1
        if len(query_ref) != n or rbuf.size < roff[-1] or qbuf.size < qoff[-1]:
            raise ValueError("fit_batch_flat: buffers, offsets and reference indices do not agree")
        qref = np.ascontiguousarray(query_ref, dtype=np.int32).reshape(-1) if n else np.zeros(1, dtype=np.int32)
        score, start, end, status = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(4))
        counts = np.zeros((max(n, 1), 4), dtype=np.int32)
        m, x, go, ge = (int(v) for v in scores)
        rc = self._L.rd_fit_batch(self._h, _p(rbuf), _p(roff), len(roff) - 1, _p(qbuf), _p(qoff), _p(qref), n, m, x, go, ge, int(budget_bytes),
                                  _p(score), _p(start), _p(end), _p(counts), _p(status))
        if rc != 0 and not (allow_too_large and rc == -4 and (status[:n] == FIT_TOO_LARGE).any()):
            self._check(rc)
        return FitResult(score[:n], start[:n], end[:n], counts[:n], status[:n])

    # ------------------------------------------------------------------ reads onto transcripts (radian_amd/map.py)
    def map_index(self, codes, offsets, k=14, w=8, max_occ=500):
        """The seed index of the transcripts in codes / offsets (lm.read_fasta's arrays), built on the device and kept in this context
        (rd_map_index).  Returns {entries, keys, keys_dropped, stage_us}."""
        codes, offsets = self._records(codes, offsets)
        st = np.zeros(8, dtype=np.int64)
        self._check(self._L.rd_map_index(self._h, _p(codes), _p(offsets), len(offsets) - 1, int(k), int(w), int(max_occ), _p(st)))
        return {"entries": int(st[0]), "keys": int(st[1]), "keys_dropped": int(st[2]), "stage_us": {"seeds": int(st[3]), "sort": int(st[4])}}

    def map_batch(self, reads, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, budget_bytes=0, allow_too_large=False, with_stats=False):
        """Map reads (code sequences 0..3, anything else a break) against the context's index (rd_map_batch): seeds, anchors, chains, the
        best and second-best transcript of every read.  budget_bytes: the anchor workspace of one launch, 0 = a quarter of free memory.  A
        read that does not fit it raises, unless allow_too_large: it then comes back with MAP_TOO_LARGE."""
        buf, off = _concat_codes(reads)
        return self.map_batch_flat(buf, off, min_anchors, min_score, max_gap, bandwidth, budget_bytes, allow_too_large, with_stats)

    def map_batch_flat(self, buf, off, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, budget_bytes=0, allow_too_large=False, with_stats=False):
        """map_batch on the C ABI's own layout: codes back to back (uint8) and int64 offsets with count + 1 entries"""
        buf, off = np.ascontiguousarray(buf, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        if buf.size < off[-1]:
            raise ValueError("map_batch_flat: the offsets end beyond the buffer")
        if buf.size == 0:
            buf = np.zeros(1, dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.int32)
        hits = np.zeros((max(n, 1), 8), dtype=np.int32)
        st = np.zeros(16, dtype=np.int64) if with_stats else None
        rc = self._L.rd_map_batch(self._h, _p(buf), _p(off), n, int(min_anchors), int(min_score), int(max_gap), int(bandwidth), int(budget_bytes),
                                  _p(status), _p(hits), _p(st))
        if rc != 0 and not (allow_too_large and rc == -4 and (status[:n] == MAP_TOO_LARGE).any()):
            self._check(rc)
        stats = None
        if with_stats:
            names = ("seeds", "lookup", "fill", "sort", "chain", "best")
            stats = {"launches": int(st[0]), "minimizers": int(st[1]), "anchors": int(st[2]), "segments": int(st[3]),
                     "stage_us": {nm: int(st[8 + i]) for i, nm in enumerate(names)}}
        return MapResult(status[:n], hits[:n], stats)

    def map_candidates(self, reads, max_cand=16, min_frac_q10=922, max_3p=-1, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, budget_bytes=0,
                       allow_too_large=False, with_stats=False):
        """The max_cand best qualifying chains of every read against the context's index (rd_map_candidates): those
        within min_frac_q10 / 1024 of the read's best score and, with max_3p >= 0, ending at most max_3p bases before the transcript's 3'
        end.  Budget and allow_too_large as map_batch.  -> CandResult."""
        buf, off = _concat_codes(reads)
        n, K = len(off) - 1, int(max_cand)
        rows = max(K, 1) if 1 <= K <= 64 else 1
        status = np.zeros(max(n, 1), dtype=np.int32)
        n_qual, n_cand = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        cands = np.zeros((max(n, 1), rows, 8), dtype=np.int32)
        st = np.zeros(16, dtype=np.int64) if with_stats else None
        rc = self._L.rd_map_candidates(self._h, _p(buf), _p(off), n, int(min_anchors), int(min_score), int(max_gap), int(bandwidth), int(budget_bytes), K,
                                       int(min_frac_q10), int(max_3p), _p(status), _p(n_qual), _p(n_cand), _p(cands), _p(st))
        if rc != 0 and not (allow_too_large and rc == -4 and (status[:n] == MAP_TOO_LARGE).any()):
            self._check(rc)
        stats = None
        if with_stats:
            names = ("seeds", "lookup", "fill", "sort", "chain", "best", "candidates")
            stats = {"launches": int(st[0]), "minimizers": int(st[1]), "anchors": int(st[2]), "segments": int(st[3]),
                     "stage_us": {nm: int(st[8 + i]) for i, nm in enumerate(names)}}
        return CandResult(status[:n], n_qual[:n], n_cand[:n], cands[:n], stats)

    def quant_em(self, cand_off, cand_t, cand_w, n_tx, max_iter=1000, tol_q20=1024, with_share=True):
        """The integer EM over every read's candidate transcripts on the GPU (rd_quant_em): cand_off int64
        [n_reads + 1], cand_t (transcripts, distinct within a read, at most 64 per read) and cand_w (weights 1..4096) per slot.
        -> QuantResult."""
        off, t, w, slots, count, share = _quant_args(cand_off, cand_t, cand_w, n_tx, with_share)
        st = np.zeros(16, dtype=np.int64)
        self._check(self._L.rd_quant_em(self._h, _p(off), _p(t), _p(w), off.size - 1, int(n_tx), int(max_iter), int(tol_q20), _p(count), _p(share), _p(st)))
        return QuantResult(count[:int(n_tx)], None if share is None else share[:slots], st)

    quant_em_host = staticmethod(quant_em_host)
    quant_workspace_bytes = staticmethod(quant_workspace_bytes)

    def map_diag_minimizers(self, codes, offsets, k, w):
        """rd_map_diag_minimizers (tests): the device's seed stage alone.  Ascending positions (uint32) of the minimizers in the flat image
        of the records, where record r starts at offsets[r] + r."""
        codes, offsets = self._records(codes, offsets)
        cap = int(offsets[-1]) + len(offsets)
        pos = np.zeros(cap, dtype=np.uint32)
        got = ctypes.c_int64(0)
        self._check(self._L.rd_map_diag_minimizers(self._h, _p(codes), _p(offsets), len(offsets) - 1, int(k), int(w), _p(pos), cap, ctypes.byref(got)))
        return pos[: got.value].copy()

    def map_diag_chain(self, t, r, q, k, min_anchors=3, max_gap=1000, bandwidth=500):
        """rd_map_diag_chain (tests): the device's chain stage alone on anchors in strictly ascending (t, r, q) order.  int32 [segments, 5]:
        the segment's first anchor, score, and the chain's first anchor, anchor count and last anchor (indices within the segment)."""
        t, r, q = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (t, r, q))
        n = t.size
        if r.size != n or q.size != n:
            raise ValueError("map_diag_chain: t, r and q differ in length")
        seg = np.zeros((max(n, 1), 5), dtype=np.int32)
        got = ctypes.c_int64(0)
        self._check(self._L.rd_map_diag_chain(self._h, _p(t), _p(r), _p(q), n, int(k), int(min_anchors), int(max_gap), int(bandwidth), _p(seg), seg.shape[0],
                                              ctypes.byref(got)))
        return seg[: got.value].copy()

    def score_math(self, which, x, y=None):
        """rd_diag_score_math (tests): one routine of the beam search's score arithmetic (SM_*) on the device, element by element.  float64
        [n]; for SM_COUNT4_GT x holds 4 n keys and y the n keys they are counted against."""
        x, y, n = _score_math_args(which, x, y)
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._check(self._L.rd_diag_score_math(self._h, int(which), _p(x), _p(y), n, _p(out)))
        return out[:n]

    @staticmethod
    def map_minimizers(codes, k, w):
        """rd_map_minimizers (host): see backend.map_minimizers"""
        return map_minimizers(codes, k, w)

    @staticmethod
    def tfrecord_write(path, signals, input_len, labels, label_len=None, append=False):
        """rd_tfrecord_write (host): see backend.tfrecord_write"""
        tfrecord_write(path, signals, input_len, labels, label_len, append)

    # ------------------------------------------------------------------ model evaluation on labelled windows (val_loss)
    def _ctc(self, fn, data, input_len, labels, label_len, with_greedy, n=None):
        n = data.shape[0] if n is None else n
        il = np.ascontiguousarray(input_len, dtype=np.int32).reshape(-1)
        if il.size != n:
            raise ValueError(f"{il.size} input lengths for {n} windows")
        lab, off, ll = _pack_labels(labels, label_len, n)
        loss = np.zeros(n, dtype=np.float64)
        status = np.zeros(n, dtype=np.int32)
        glen = np.zeros(n, dtype=np.int32)
        ed = np.zeros(n, dtype=np.int32)
        g = np.zeros((n, CTC_T), dtype=np.uint8) if with_greedy else None
        self._check(fn(self._h, data if isinstance(data, ctypes.c_void_p) else _p(data), n, _p(il), _p(lab), _p(off), _p(ll), _p(loss), _p(status), _p(glen), _p(ed), _p(g)))
        greedy = [g[i, : glen[i]].copy() for i in range(n)] if with_greedy else None
        return CtcResult(loss, status, glen, ed, greedy)

    def ctc_eval(self, windows, input_len, labels, label_len=None, with_greedy=False):
        """Keras ctc_batch_cost on the loaded weights' softmax rows (radian/model.py:77-98) plus a greedy edit distance, on the GPU
        (rd_ctc_eval: forward -> CTC -> greedy / Levenshtein).  windows [n, 1024] float32; input_len [n]; labels [n, Lmax] or a list
        of sequences of 0..3 with label_len [n] of them counted (None: all).  Returns a CtcResult."""
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        if windows.ndim != 2 or windows.shape[1] != CTC_T:
            raise ValueError(f"windows must be [n_windows, {CTC_T}]")
        return self._ctc(self._L.rd_ctc_eval, windows, input_len, labels, label_len, with_greedy)

    def ctc_probs(self, probs, input_len, labels, label_len=None, with_greedy=False):
        """the same on caller-supplied softmax rows probs [n, 1024, 5] float32 (rd_ctc_probs)"""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        if probs.ndim != 3 or probs.shape[1:] != (CTC_T, 5):
            raise ValueError(f"probs must be [n_windows, {CTC_T}, 5]")
        return self._ctc(self._L.rd_ctc_probs, probs, input_len, labels, label_len, with_greedy)

    def ctc_probs_resident(self, d_probs, n, input_len, labels, label_len=None, with_greedy=False):
        """the same on n windows of rows already in device memory (rd_ctc_probs_resident; d_probs from dev_alloc)"""
        return self._ctc(self._L.rd_ctc_probs_resident, d_probs, input_len, labels, label_len, with_greedy, n=int(n))

    # ------------------------------------------------------------------ training (radian/train.py: model.fit with ctc_batch_cost and Adam)
    def _train_args(self, n, input_len, labels, label_len):
        il = np.ascontiguousarray(input_len, dtype=np.int32).reshape(-1)
        if il.size != n:
            raise ValueError(f"{il.size} input lengths for {n} windows")
        lab, off, ll = _pack_labels(labels, label_len, n)
        return il, lab, off, ll, np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)

    @staticmethod
    def _windows(windows):
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        if windows.ndim != 2 or windows.shape[1] != CTC_T:
            raise ValueError(f"windows must be [n_windows, {CTC_T}]")
        return windows

    def train_grad(self, windows, input_len, labels, label_len=None):
        """(grad float32 [n_params] in load_weights order, loss float64 [n], status int32 [n]): the gradient of the batch's mean
        Keras ctc_batch_cost on the loaded weights (rd_train_grad; infeasible windows give zero loss and gradient, the mean divides by n)"""
        windows = self._windows(windows)
        n = windows.shape[0]
        il, lab, off, ll, loss, status = self._train_args(n, input_len, labels, label_len)
        grad = np.zeros(self._param_count(), dtype=np.float32)
        self._check(self._L.rd_train_grad(self._h, _p(windows), n, _p(il), _p(lab), _p(off), _p(ll), _p(grad), _p(loss), _p(status)))
        return grad, loss, status

    def train_step(self, windows, input_len, labels, label_len=None, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7, resident_n=None):
        """One Adam step on the batch, in place on the context's weights (rd_train_step; rd_train_step_resident when windows is a
        device pointer and resident_n its window count).  Returns (loss float64 [n], status int32 [n]) before the update."""
        opt = _Adam(lr, beta1, beta2, epsilon)
        if resident_n is not None:
            n = int(resident_n)
            il, lab, off, ll, loss, status = self._train_args(n, input_len, labels, label_len)
            self._check(self._L.rd_train_step_resident(self._h, windows, n, _p(il), _p(lab), _p(off), _p(ll), ctypes.byref(opt), _p(loss),
                                                       _p(status)))
            return loss, status
        windows = self._windows(windows)
        n = windows.shape[0]
        il, lab, off, ll, loss, status = self._train_args(n, input_len, labels, label_len)
        self._check(self._L.rd_train_step(self._h, _p(windows), n, _p(il), _p(lab), _p(off), _p(ll), ctypes.byref(opt), _p(loss), _p(status)))
        return loss, status

    def train_reset(self):
        """Adam's moments and step count to zero (rd_train_reset)"""
        self._check(self._L.rd_train_reset(self._h))

    def get_weights(self):
        """the context's current weights, flat float32 in load_weights order (rd_get_weights)"""
        out = np.zeros(self._param_count(), dtype=np.float32)
        self._check(self._L.rd_get_weights(self._h, _p(out), out.size))
        return out

    def _param_count(self):
        """the loaded model's parameter count, from the library (weights may have arrived by rd_clone_artifacts / rd_rccl_bcast_model)"""
        n = ctypes.c_int64(0)
        self._check(self._L.rd_model_params(self._h, ctypes.byref(n)))
        return n.value

    def train_ctc_grad(self, probs, input_len, labels, label_len=None):
        """(grad_z float32 [n, 1024, 5], loss float64 [n], status int32 [n]): dL/dz of the batch's mean loss on caller-supplied softmax
        rows probs [n, 1024, 5] (rd_train_ctc_grad: the CTC part of train_grad alone)"""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        if probs.ndim != 3 or probs.shape[1:] != (CTC_T, 5):
            raise ValueError(f"probs must be [n_windows, {CTC_T}, 5]")
        n = probs.shape[0]
        il, lab, off, ll, loss, status = self._train_args(n, input_len, labels, label_len)
        gz = np.zeros_like(probs)
        self._check(self._L.rd_train_ctc_grad(self._h, _p(probs), n, _p(il), _p(lab), _p(off), _p(ll), _p(gz), _p(loss), _p(status)))
        return gz, loss, status


class _Adam(ctypes.Structure):
    """rd_adam (include/radian_hip.h)"""
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("epsilon", ctypes.c_float)]
