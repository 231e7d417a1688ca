"""Host-side mirror of the gmove seam over libpgmove's C ABI (include/pgmove.h).

Names follow the reference's vocabulary (reads, ss ops, k-mer slice, slots, dump events); see
src/gmove.cpp:707-975 of hiruna72/poregen for the loop this replaces. All computation happens in
libpgmove.so on the GPU; this module only marshals pointers (numpy arrays for host batches, torch
tensors for device-resident batches).
"""
import ctypes as C
import itertools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _abi


class PgError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"libpgmove status {status}: {text}")
        self.status = status
        self.text = text


def generate_kmers(k: int, rna: bool = False) -> List[str]:
    """Lexicographic 4^k k-mers over ACGT / ACGU (generate_kmers, src/poregen.cpp:248-267)."""
    return ["".join(t) for t in itertools.product("ACGU" if rna else "ACGT", repeat=k)]


def reconcile_slice(n_kmers: int, index_start: int = 1, index_end: int = 500, file_limit: int = 500):
    """The slice reconciliation of gmove() (src/gmove.cpp:428-440) -> final (index_start, index_end)."""
    if file_limit < n_kmers:
        pass
    elif file_limit > n_kmers - index_start + 1:
        if index_end > n_kmers:
            file_limit = n_kmers - index_start + 1
            index_end = index_start + file_limit - 1
    return index_start, index_end


@dataclass
class GmoveParams:
    kmers: Sequence[str]                 # the k-mer slice, in list order: slot i = kmers[i]
    kmer_size: int = 9
    sig_move_offset: int = 0
    margin: int = 0
    sample_limit: int = 100
    max_dur: int = 70
    min_dur: int = 5
    kmer_pick_margin: int = 2
    scaling: int = 0
    rna: bool = False
    pa_min: float = 40.0
    pa_max: float = 180.0
    device: int = 0
    lazy_stats: bool = False
    profile: bool = False
    overlap: Optional[bool] = None       # None: the library's default (two streams when it computes eager statistics); True / False: PG_FLAG_OVERLAP / PG_FLAG_ONE_STREAM
    debug_narrow: bool = False
    overlap_tail: bool = False           # statistics on a second stream next to pg_collect's small launches (PG_FLAG_OVERLAP_TAIL)
    split_walk: bool = False             # measurement/tests: ss walk and event filter as two launches (PG_FLAG_DEBUG_SPLIT_WALK)
    defer_stats: bool = False            # multi-GPU step: the statistics are queued by stats() (behind the issue of the collective) or by collect()
    stop_when_full: bool = False         # kmers is the WHOLE list: errors behind the read that completes the last k-mer do not count


_BATCH_FIELDS = [
    ("sig", np.int16), ("sig_off", np.uint64), ("digitisation", np.float64), ("offset", np.float64),
    ("range", np.float64), ("query_start", np.int32), ("target_start", np.int32), ("target_end", np.int32),
    ("seq", np.uint8), ("seq_off", np.uint64), ("op_n", np.uint32), ("op_t", np.uint8), ("op_off", np.uint64),
]


@dataclass
class Batch:
    """One batch of reads in PAF-line order (layout: pg_batch in include/pgmove.h)."""
    n_reads: int
    sig: object
    sig_off: object
    digitisation: object
    offset: object
    range: object
    query_start: object
    target_start: object
    target_end: object
    seq: object
    seq_off: object
    op_n: object
    op_t: object
    op_off: object
    on_device: bool = False
    n_ops: int = 0   # device batches: op_off[n_reads] when known (pg_batch.n_ops); 0 = the library reads it back (one sync per call)
    all_matches: bool = False  # the batch holds match ops only and the caller vouches for it (PG_BATCH_ALL_MATCHES, verified on the device)
    resident: bool = False     # device batch, engine on the caller's stream: nothing queued on that stream produces the arrays (PG_BATCH_RESIDENT)
    gapped: bool = False       # ModelFit / Realigner: ops on the signal-to-reference alignment (op_t 0 match, 1 I, 2 D), seq the reference slices (PG_BATCH_GAPPED)

    def validate_host(self):
        for name, dt in _BATCH_FIELDS:
            a = getattr(self, name)
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags["C_CONTIGUOUS"], (name, getattr(a, "dtype", None))
        return self

    def to_device(self, device):
        import torch
        kw = {}
        for name, dt in _BATCH_FIELDS:
            a = getattr(self, name)
            # torch has no uint64/uint32: ship the bytes as int64/int32 of the same width
            view = {np.uint64: np.int64, np.uint32: np.int32}.get(dt, dt)
            t = torch.from_numpy(np.ascontiguousarray(a).view(view))
            if name == "sig":  # 16-byte slack so the tail vector of the last read stays inside the allocation
                t = torch.cat([t, torch.zeros(8, dtype=t.dtype)])
            kw[name] = t.to(device)
        return Batch(n_reads=self.n_reads, on_device=True, n_ops=int(self.op_off[-1]), all_matches=not self.gapped and not bool(np.any(self.op_t)), gapped=self.gapped, **kw)

    def slice_reads(self, lo: int, hi: int) -> "Batch":
        """Host batch holding reads [lo, hi) (used to shard a PAF-ordered batch across ranks)."""
        assert not self.on_device
        so, qo, oo = self.sig_off, self.seq_off, self.op_off
        return Batch(
            n_reads=hi - lo,
            sig=np.ascontiguousarray(self.sig[int(so[lo]):int(so[hi])]), sig_off=(so[lo:hi + 1] - so[lo]).astype(np.uint64),
            digitisation=np.ascontiguousarray(self.digitisation[lo:hi]), offset=np.ascontiguousarray(self.offset[lo:hi]),
            range=np.ascontiguousarray(self.range[lo:hi]), query_start=np.ascontiguousarray(self.query_start[lo:hi]),
            target_start=np.ascontiguousarray(self.target_start[lo:hi]), target_end=np.ascontiguousarray(self.target_end[lo:hi]),
            seq=np.ascontiguousarray(self.seq[int(qo[lo]):int(qo[hi])]), seq_off=(qo[lo:hi + 1] - qo[lo]).astype(np.uint64),
            op_n=np.ascontiguousarray(self.op_n[int(oo[lo]):int(oo[hi])]), op_t=np.ascontiguousarray(self.op_t[int(oo[lo]):int(oo[hi])]),
            op_off=(oo[lo:hi + 1] - oo[lo]).astype(np.uint64))

    @property
    def n_samples(self) -> int:
        return int(self.sig_off[-1]) if not self.on_device else int(self.sig_off[-1].item())


@dataclass
class Result:
    counts: np.ndarray
    ev_off: np.ndarray
    ev_len: np.ndarray
    ev_read: np.ndarray
    samp_off: np.ndarray
    samples: np.ndarray
    read_skipped: np.ndarray
    n_reads: int

    def slot_values(self, s: int) -> np.ndarray:
        a, b = int(self.ev_off[s]), int(self.ev_off[s + 1])
        return self.samples[int(self.samp_off[a]):int(self.samp_off[b])]

    def slot_text(self, s: int, delimit: bool = False, sample_limit: Optional[int] = None) -> str:
        """dump/<KMER> content (src/gmove.cpp:941-944, 196-203) -- test helper; the CLI formats in C++."""
        out = []
        a, b = int(self.ev_off[s]), int(self.ev_off[s + 1])
        closed_at = None
        if sample_limit is not None and b - a == sample_limit and sample_limit > 0:
            closed_at = int(self.ev_read[b - 1])
        e = a
        for r in range(self.n_reads if delimit else 0):
            while e < b and self.ev_read[e] == r:
                out.append(self._ev_text(e)); e += 1
            if not self.read_skipped[r] and (closed_at is None or r < closed_at):
                out.append(":")
        if not delimit:
            out = [self._ev_text(i) for i in range(a, b)]
        return "".join(out)

    def _ev_text(self, e: int) -> str:
        v = self.samples[int(self.samp_off[e]):int(self.samp_off[e + 1])]
        return ",".join("%.8f" % x for x in v) + ";"


@dataclass
class Model:
    """pg_model_result as numpy arrays (one entry per slot) plus datamash-formatted texts."""
    n_values: np.ndarray
    median: np.ndarray
    sstdev: np.ndarray
    mid_lo: np.ndarray
    mid_hi: np.ndarray
    origin: np.ndarray
    sum1: np.ndarray
    sum2_lo: np.ndarray
    sum2_hi: np.ndarray
    dwell_n: np.ndarray
    dwell_median: np.ndarray
    median_text: List[str]
    sstdev_text: List[str]
    dwell_text: List[str]

    def raw_model_lines(self, kmers: List[str], limit: str = "3.1") -> str:
        """The file calculate_mean_stddev_all writes (scripts/poregen.sh:54-85): sorted by name, stddev capped."""
        out = []
        for i in sorted(range(len(kmers)), key=lambda j: kmers[j]):
            sd = self.sstdev_text[i]
            if sd not in ("", "nan") and float(sd) > float(limit):
                sd = limit
            out.append(f"{kmers[i]}\t{self.median_text[i]}\t{sd}\n")
        return "".join(out)

    def dwell_lines(self, kmers: List[str]) -> str:
        return "".join(f"{kmers[i]}\t{self.dwell_text[i]}\n" for i in sorted(range(len(kmers)), key=lambda j: kmers[j]))


@dataclass
class EventModel:
    """The event table (pg_dmodel_finish_events / pg_model_events): `means` and `sds` are Models with one entry per file or slot -- the
    reduction of its events' means and of its events' standard deviations, in 1e-8 units; a refused entry reads as empty."""
    means: "Model"
    sds: "Model"
    status: np.ndarray        # per entry: 0, or _abi.PG_EVENTS_* bits of its refusal
    n_events: np.ndarray
    refusal: list             # per entry: the message, "" when not refused
    ev_mean: object           # DumpModel(events=True, keep_events=True): every event's mean / standard deviation, entry after entry, else None
    ev_sd: object
    event_ms: float           # DumpModel(profile=True): device time of the per-event kernels / of the two reductions behind them
    reduce_ms: float

    def lines(self, names) -> str:
        """NAME<TAB>n_events<TAB>mean_median<TAB>mean_sstdev<TAB>sd_median<TAB>sd_sstdev, sorted by name; ValueError for a refused entry"""
        out = []
        for i in sorted(range(len(names)), key=lambda j: names[j].encode()):
            if self.status[i]:
                raise ValueError("the event table of %s is refused: %s" % (names[i], self.refusal[i]))
            out.append("%s\t%d\t%s\t%s\t%s\t%s\n" % (names[i], int(self.n_events[i]), self.means.median_text[i], self.means.sstdev_text[i],
                                                     self.sds.median_text[i], self.sds.sstdev_text[i]))
        return "".join(out)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


def _fill_params(owner, lib, params: "GmoveParams"):
    """pg_params for `params`; the code -> slot tables are kept alive on `owner`."""
    n_slots = len(params.kmers)
    k = params.kmer_size
    n_codes = 4 ** k
    owner._table_t = np.empty(n_codes, dtype=np.int32)
    owner._table_u = np.empty(n_codes, dtype=np.int32)
    arr = (C.c_char_p * n_slots)(*[s.encode() for s in params.kmers])
    st = lib.pg_build_slot_tables(k, arr, n_slots, owner._table_t.ctypes.data, owner._table_u.ctypes.data)
    if st != 0:
        raise PgError(st, lib.pg_last_error(None).decode())
    p = _abi.PgParams()
    lib.pg_default_params(C.byref(p))
    p.kmer_size = k; p.sig_move_offset = params.sig_move_offset; p.signal_print_margin = params.margin
    p.sample_limit = params.sample_limit; p.max_dur = params.max_dur; p.min_dur = params.min_dur
    p.kmer_pick_margin = params.kmer_pick_margin; p.scaling = params.scaling; p.allow_rna = int(params.rna)
    p.pa_min = params.pa_min; p.pa_max = params.pa_max; p.n_slots = n_slots
    p.flags = ((_abi.PG_FLAG_LAZY_STATS if params.lazy_stats else 0) | (_abi.PG_FLAG_PROFILE if params.profile else 0)
               | (_abi.PG_FLAG_OVERLAP if params.overlap else (_abi.PG_FLAG_ONE_STREAM if params.overlap is False else 0)) | (_abi.PG_FLAG_DEBUG_NARROW if params.debug_narrow else 0)
               | (_abi.PG_FLAG_STOP_WHEN_FULL if params.stop_when_full else 0) | (_abi.PG_FLAG_DEFER_STATS if params.defer_stats else 0)
               | (_abi.PG_FLAG_DEBUG_SPLIT_WALK if params.split_walk else 0)
               | (_abi.PG_FLAG_OVERLAP_TAIL if params.overlap_tail else 0))
    p.device = params.device
    p.table_t = owner._table_t.ctypes.data; p.table_u = owner._table_u.ctypes.data
    return p


def _result_from(r) -> "Result":
    def arr(ptr, n, dt):
        if n == 0 or not ptr:
            return np.zeros(0, dtype=dt)
        buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dt).copy()
    ns, ne, nsmp, nr = r.n_slots, r.n_events, r.n_samples, r.n_reads
    return Result(counts=arr(r.counts, ns, np.uint64), ev_off=arr(r.ev_off, ns + 1, np.uint64),
                  ev_len=arr(r.ev_len, ne, np.uint32), ev_read=arr(r.ev_read, ne, np.uint32),
                  samp_off=arr(r.samp_off, ne + 1, np.uint64), samples=arr(r.samples, nsmp, np.float64),
                  read_skipped=arr(r.read_skipped, nr, np.uint8), n_reads=int(nr))


def _text_slots(owner, t, fetch):
    off = [int(t.slot_off[i]) for i in range(t.n_slots + 1)]
    buf = C.create_string_buffer(int(t.n_bytes) + 1)
    owner._check(fetch(owner._h, 0, int(t.n_bytes), buf))
    raw = buf.raw
    return [raw[off[i]:off[i + 1]] for i in range(t.n_slots)]


def _deferred_result(owner, r, fetch, piece) -> "Result":
    res = _result_from(r)
    if r.n_samples and not r.samples:  # still on the device: range by range
        smp = np.empty(int(r.n_samples), dtype=np.float64)
        for a in range(0, int(r.n_samples), piece):
            n = min(piece, int(r.n_samples) - a)
            owner._check(fetch(owner._h, a, n, smp[a:a + n].ctypes.data_as(C.c_void_p)))
        res.samples = smp
    return res


def _c_batch(b: "Batch"):
    cb = _abi.PgBatch()
    cb.struct_size = C.sizeof(_abi.PgBatch)
    cb.location = _abi.PG_LOC_DEVICE if b.on_device else _abi.PG_LOC_HOST
    cb.n_reads = b.n_reads
    cb.n_ops = b.n_ops if b.on_device else 0
    cb.flags = (_abi.PG_BATCH_ALL_MATCHES if b.all_matches else 0) | (_abi.PG_BATCH_RESIDENT if (b.resident and b.on_device) else 0) | (_abi.PG_BATCH_GAPPED if b.gapped else 0)
    for name, _ in _BATCH_FIELDS:
        setattr(cb, name, _ptr(getattr(b, name)))
    return cb


class GmoveEngine:
    """One gmove run on one GPU: the state the reference keeps in gmove() + process_move_table_paf()."""

    def __init__(self, params: GmoveParams):
        self._lib = _abi.load()
        self.params = params
        self.n_slots = len(params.kmers)
        p = _fill_params(self, self._lib, params)
        h = C.c_void_p()
        st = self._lib.pg_create(C.byref(p), C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_last_error(None).decode())
        self._h = h
        self._keep = None  # keeps the arrays of the batch between count and collect alive

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_last_error(self._h).decode())

    def _c_batch(self, b: Batch):
        return _c_batch(b)

    def _set_read_scaling(self, b: Batch, scaling):
        """scaling: a ReadScaling (ModelFit.calibrate) or (center, spread, use), three numpy arrays or three CUDA tensors of b.n_reads
        entries: the per-read scaling of the batch about to be counted, for an engine made with scaling=2 (pg_set_read_scaling)."""
        if scaling is None:
            return None
        c, s, u = (scaling.center, scaling.spread, scaling.use) if hasattr(scaling, "center") else scaling
        host = isinstance(c, np.ndarray) or not hasattr(c, "data_ptr")
        if host:
            c, s, u = np.ascontiguousarray(c, dtype=np.float64), np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(u, dtype=np.uint8)
            sizes = (c.size, s.size, u.size)
        else:
            import torch
            c, s, u = c.contiguous().to(torch.float64), s.contiguous().to(torch.float64), u.contiguous().to(torch.uint8)
            sizes = (c.numel(), s.numel(), u.numel())
        if sizes != (b.n_reads,) * 3:
            raise ValueError("scaling needs one center, spread and use per read of the batch")
        self._check(self._lib.pg_set_read_scaling(self._h, C.c_void_p(_ptr(c)), C.c_void_p(_ptr(s)), C.c_void_p(_ptr(u)), _abi.PG_LOC_HOST if host else _abi.PG_LOC_DEVICE))
        return (c, s, u, scaling)

    def submit(self, b: Batch, scaling=None):
        self._keep = (b, self._set_read_scaling(b, scaling))
        self._check(self._lib.pg_submit(self._h, C.byref(self._c_batch(b))))

    def count(self, b: Batch, out=None, scaling=None):
        """Phase 1. Returns the per-slot accepted-event counts of this batch (uncapped): a numpy uint64
        array, or fills `out` (a torch int64 CUDA tensor) in place when given."""
        self._keep = (b, self._set_read_scaling(b, scaling))
        if out is None:
            res = np.empty(self.n_slots, dtype=np.uint64)
            self._check(self._lib.pg_count(self._h, C.byref(self._c_batch(b)), res.ctypes.data, _abi.PG_LOC_HOST))
            return res
        self._check(self._lib.pg_count(self._h, C.byref(self._c_batch(b)), out.data_ptr(), _abi.PG_LOC_DEVICE))
        return out

    def stats(self):
        """Between count() and collect() of an engine made with defer_stats: queue the per-read statistics now (pg_stats)."""
        self._check(self._lib.pg_stats(self._h))

    def collect(self, base=None):
        """Phase 2. base: per-slot count of accepted events that precede this batch (numpy uint64 or a
        torch int64 CUDA tensor); None = this engine's own running count."""
        if base is None:
            self._check(self._lib.pg_collect(self._h, None, _abi.PG_LOC_HOST))
        elif isinstance(base, np.ndarray):
            base = np.ascontiguousarray(base, dtype=np.uint64)
            self._check(self._lib.pg_collect(self._h, base.ctypes.data, _abi.PG_LOC_HOST))
        else:
            self._check(self._lib.pg_collect(self._h, base.data_ptr(), _abi.PG_LOC_DEVICE))

    def collect_gathered(self, all_counts, world: int, rank: int):
        """Phase 2 of a multi-GPU job: all_counts = the all_gather's receive buffer (torch int64 CUDA tensor,
        world x n_slots, row g = rank g's count()); the library sums the rows below `rank` on its own stream."""
        if all_counts.numel() != world * self.n_slots or not all_counts.is_contiguous():
            raise ValueError("all_counts must be a contiguous world x n_slots tensor")
        self._check(self._lib.pg_collect_gathered(self._h, all_counts.data_ptr(), world, rank))

    def job_totals(self, device=None):
        """After collect_gathered: (accepted events of all ranks per slot, freq.txt values of the job) as int64 CUDA tensors that
        alias the library's buffers (pg_job_totals_device); rewritten by every collect_gathered on the engine's stream."""
        import torch
        if getattr(self, "_job_totals", None) is None:
            a, b = C.c_void_p(), C.c_void_p()
            self._check(self._lib.pg_job_totals_device(self._h, C.byref(a), C.byref(b)))
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device

            class _Alias:
                def __init__(self, ptr, n):
                    self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i8", "data": (int(ptr), False), "version": 2}
            self._job_totals = tuple(torch.as_tensor(_Alias(x.value, self.n_slots), device=dev) for x in (a, b))
        return self._job_totals

    def sync(self):
        self._check(self._lib.pg_sync(self._h))

    def use_torch_stream(self, stream=None):
        """Run the main chain on a torch CUDA stream (default: the current one) so that torch collectives
        between count() and collect() are ordered on the device, without host synchronisation."""
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        if not s.cuda_stream:
            raise ValueError("use a non-default torch stream (torch.cuda.Stream() + torch.cuda.set_stream): handle 0 means "
                             "'the context's own stream' in pg_set_stream")
        self._check(self._lib.pg_set_stream(self._h, C.c_void_p(s.cuda_stream)))

    def reset(self):
        self._check(self._lib.pg_reset(self._h))

    def all_slots_full(self) -> bool:
        return bool(self._lib.pg_all_slots_full(self._h))

    def finish(self) -> Result:
        r = _abi.PgResult()
        self._check(self._lib.pg_finish(self._h, C.byref(r)))
        return _result_from(r)

    def model(self, keep_first: bool = False) -> "Model":
        """Per-k-mer median / sample stddev / dwell median of everything collected so far, reduced on the device from
        the kept samples (pg_model): the values `scripts/poregen.sh:54-85,33-52` derive from the dump files with
        tr | tail | datamash. `text(slot, which)` gives the number exactly as datamash prints it."""
        m = _abi.PgModelResult()
        self._check(self._lib.pg_model(self._h, _abi.PG_MODEL_KEEP_FIRST if keep_first else 0, C.byref(m)))
        return self._model_from(m)

    def model_events(self) -> "EventModel":
        """The event table of everything collected so far (pg_model_events): per k-mer the reduction of its kept events' means and of their
        standard deviations, the numbers `poregen model --event_model` derives from the dump files."""
        r = _abi.PgEventsResult()
        self._check(self._lib.pg_model_events(self._h, 0, C.byref(r)))
        ns = r.means.n_slots
        status = np.ctypeslib.as_array(C.cast(r.status, C.POINTER(C.c_uint32)), (ns,)).copy() if ns else np.zeros(0, np.uint32)
        n_events = np.ctypeslib.as_array(C.cast(r.n_events, C.POINTER(C.c_uint64)), (ns,)).copy() if ns else np.zeros(0, np.uint64)
        return EventModel(means=self._model_from(r.means), sds=self._model_from(r.sds), status=status, n_events=n_events,
                          refusal=[self._lib.pg_events_status_text(int(x)).decode() for x in status], ev_mean=None, ev_sd=None, event_ms=0.0, reduce_ms=0.0)

    def model_device(self, counts, ev_len, samples, keep_first: bool = False) -> "Model":
        """The same reduction over torch CUDA tensors in the layout `dist.gather_kept` returns on the writing rank: counts
        int64[n_slots] kept events per k-mer, ev_len int32/uint32[n_events] (k-mer-major), samples float64[] back to back
        (pg_model_device)."""
        import torch
        ev_off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
        ev_off[1:] = torch.cumsum(counts.to(torch.int64), 0)
        samp_off = torch.zeros(ev_len.numel() + 1, dtype=torch.int64, device=counts.device)
        samp_off[1:] = torch.cumsum(ev_len.to(torch.int64), 0)
        ev_len = ev_len.contiguous(); samples = samples.contiguous()
        assert ev_len.element_size() == 4 and samples.dtype == torch.float64 and int(samp_off[-1]) == samples.numel()
        torch.cuda.current_stream(counts.device).synchronize()   # the library launches on its own stream
        m = _abi.PgModelResult()
        self._check(self._lib.pg_model_device(self._h, counts.numel(), ev_off.data_ptr(), samp_off.data_ptr(), ev_len.data_ptr() or None,
                                              samples.data_ptr() or None, _abi.PG_MODEL_KEEP_FIRST if keep_first else 0, C.byref(m)))
        return self._model_from(m)

    def _model_from(self, m) -> "Model":
        ns = m.n_slots

        def arr(ptr, dt):
            if ns == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.frombuffer((C.c_char * (ns * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy()
        buf = C.create_string_buffer(64)
        texts = []
        for which in (_abi.PG_MODEL_TEXT_MEDIAN, _abi.PG_MODEL_TEXT_SSTDEV, _abi.PG_MODEL_TEXT_DWELL):
            col = []
            for s in range(ns):
                n = self._lib.pg_model_format(C.byref(m), s, which, buf, 64)
                col.append(buf.raw[:n].decode())
            texts.append(col)
        return Model(n_values=arr(m.n_values, np.uint64), median=arr(m.median, np.float64), sstdev=arr(m.sstdev, np.float64),
                     mid_lo=arr(m.mid_lo, np.int64), mid_hi=arr(m.mid_hi, np.int64), origin=arr(m.origin, np.int64),
                     sum1=arr(m.sum1, np.int64), sum2_lo=arr(m.sum2_lo, np.uint64), sum2_hi=arr(m.sum2_hi, np.uint64),
                     dwell_n=arr(m.dwell_n, np.uint64), dwell_median=arr(m.dwell_median, np.float64),
                     median_text=texts[0], sstdev_text=texts[1], dwell_text=texts[2])

    def text(self):
        """The dump files' text produced on the device (pg_text): list of bytes objects, one per slot -- what the reference's fprintf calls
        write into dump/<KMER> without -d."""
        t = _abi.PgTextResult()
        self._check(self._lib.pg_text(self._h, C.byref(t)))
        return _text_slots(self, t, self._lib.pg_fetch_text)

    def text_device_offsets(self, counts, ev_len, samples) -> np.ndarray:
        """pg_text_device over torch CUDA tensors in model_device's layout (counts int64[n_slots], ev_len int32/uint32[n_events],
        samples float64[]): produces the text on the device and returns slot_off (uint64[n_slots + 1]; slot s is bytes
        [slot_off[s], slot_off[s+1]) of fetch_text, slot_off[-1] the total). The text stays valid until the context's next text call."""
        import torch
        ev_off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
        ev_off[1:] = torch.cumsum(counts.to(torch.int64), 0)
        samp_off = torch.zeros(ev_len.numel() + 1, dtype=torch.int64, device=counts.device)
        samp_off[1:] = torch.cumsum(ev_len.to(torch.int64), 0)
        samples = samples.contiguous()
        assert samples.dtype == torch.float64 and int(samp_off[-1]) == samples.numel() and int(ev_off[-1]) == ev_len.numel()
        torch.cuda.current_stream(counts.device).synchronize()   # the library launches on its own stream
        t = _abi.PgTextResult()
        self._check(self._lib.pg_text_device(self._h, counts.numel(), ev_len.numel(), ev_off.data_ptr(), samp_off.data_ptr(),
                                             samples.data_ptr() or None, C.byref(t)))
        off = np.ctypeslib.as_array(t.slot_off, shape=(t.n_slots + 1,)).copy()
        assert int(off[-1]) == int(t.n_bytes)
        return off

    def fetch_text(self, first: int, n: int) -> bytes:
        """bytes [first, first + n) of the context's last text (pg_fetch_text)"""
        buf = C.create_string_buffer(n + 1)
        self._check(self._lib.pg_fetch_text(self._h, first, n, buf))
        return buf.raw[:n]

    def text_device(self, counts, ev_len, samples) -> List[bytes]:
        """The dump files' text of device arrays (text_device_offsets): one bytes object per slot."""
        off = self.text_device_offsets(counts, ev_len, samples)
        raw = self.fetch_text(0, int(off[-1]))
        return [raw[int(off[s]):int(off[s + 1])] for s in range(off.size - 1)]

    def finish_deferred(self, piece: int = 1 << 20) -> Result:
        """pg_finish_deferred + pg_fetch_samples: the same Result as finish(), the samples fetched from the device `piece` at a time."""
        r = _abi.PgResult()
        self._check(self._lib.pg_finish_deferred(self._h, C.byref(r)))
        return _deferred_result(self, r, self._lib.pg_fetch_samples, piece)

    def device_view(self):
        v = _abi.PgDeviceView()
        self._check(self._lib.pg_last_batch_device(self._h, C.byref(v)))
        return v

    def kept_tensors(self, device=None, with_reads=False):
        """The last collected batch as torch CUDA tensors that alias the library's device buffers (valid until the next
        submit/collect/reset): (kept events per slot int64[n_slots], window lengths int32[n_events] in slot-major
        order, samples float64[n_samples]; with_reads: also the kept events' read indices inside the batch, int32[n_events]). What
        dist.gather_kept sends to the writing rank."""
        import torch
        v = self.device_view()

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device

        def wrap(ptr, n, typestr, dtype):
            if n == 0 or not ptr:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_Alias(ptr, n, typestr), device=dev)

        counts = wrap(v.d_keep, self.n_slots, "<i8", torch.int64)
        ev_len = wrap(v.d_ev_len, v.n_events, "<i4", torch.int32)
        samples = wrap(v.d_samples, v.n_samples, "<f8", torch.float64)
        if with_reads:
            return counts, ev_len, samples, wrap(v.d_ev_read, v.n_events, "<i4", torch.int32)
        return counts, ev_len, samples

    def kernel_stats(self):
        n = C.c_uint32(0)
        buf = (_abi.PgKernelStat * 64)()
        self._check(self._lib.pg_kernel_stats(self._h, buf, 64, C.byref(n)))
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(min(n.value, 64))}

    def kernel_stats_reset(self):
        self._check(self._lib.pg_kernel_stats_reset(self._h))


class GmoveJob:
    """One gmove job over several GPUs from THIS process (pg_job_*): the batch is cut into contiguous shards, one per listed
    device, with one exchange of per-k-mer counts per batch (RCCL all-gather when the devices are distinct, host memory
    otherwise). Same results as a GmoveEngine fed the same batches."""

    def __init__(self, params: GmoveParams, devices: Sequence[int], exchange: int = _abi.PG_JOB_EXCHANGE_AUTO):
        self._lib = _abi.load()
        self.params = params
        self.n_slots = len(params.kmers)
        p = _fill_params(self, self._lib, params)
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        st = self._lib.pg_job_create(C.byref(p), devs, len(devices), exchange, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_job_last_error(None).decode())
        self._h = h
        self._keep = None

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_job_last_error(self._h).decode())

    @property
    def uses_rccl(self) -> bool:
        return bool(self._lib.pg_job_uses_rccl(self._h))

    def submit(self, b: Batch):
        self._keep = b
        self._check(self._lib.pg_job_submit(self._h, C.byref(_c_batch(b))))

    def submit_shards(self, shards: Sequence[Batch]):
        """pg_job_submit_shards: one batch per device of the job, in PAF order, each where it will be worked (a device batch resident
        on that device, or a host batch): nothing is cut or copied on the host."""
        self._keep = list(shards)
        arr = (_abi.PgBatch * len(shards))(*[_c_batch(b) for b in shards])
        self._check(self._lib.pg_job_submit_shards(self._h, arr, len(shards)))

    def reset(self):
        self._check(self._lib.pg_job_reset(self._h))

    def sync(self):
        self._check(self._lib.pg_job_sync(self._h))

    def all_slots_full(self) -> bool:
        return bool(self._lib.pg_job_all_slots_full(self._h))

    def finish(self) -> Result:
        r = _abi.PgResult()
        self._check(self._lib.pg_job_finish(self._h, C.byref(r)))
        return _result_from(r)

    def finish_deferred(self, piece: int = 1 << 20) -> Result:
        """pg_job_finish_deferred + pg_job_fetch_samples: the shards' samples concatenated on the job's first device, fetched in pieces."""
        r = _abi.PgResult()
        self._check(self._lib.pg_job_finish_deferred(self._h, C.byref(r)))
        return _deferred_result(self, r, self._lib.pg_job_fetch_samples, piece)

    def text(self):
        """pg_job_text: the dump files' text of the whole job, produced on its first device; one bytes object per slot."""
        t = _abi.PgTextResult()
        self._check(self._lib.pg_job_text(self._h, C.byref(t)))
        return _text_slots(self, t, self._lib.pg_job_fetch_text)

    def model(self, keep_first: bool = False) -> "Model":
        m = _abi.PgModelResult()
        self._check(self._lib.pg_job_model(self._h, _abi.PG_MODEL_KEEP_FIRST if keep_first else 0, C.byref(m)))
        return GmoveEngine._model_from(self, m)

    def kernel_stats(self, shard: int):
        """pg_kernel_stats of one shard's context (params.profile): {kernel: (launches, total ms)}."""
        n = C.c_uint32(0)
        buf = (_abi.PgKernelStat * 64)()
        self._check(self._lib.pg_job_kernel_stats(self._h, shard, buf, 64, C.byref(n)))
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(min(n.value, 64))}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- kmer_freq ------------------------------------------------------------------------------------------------------------------

@dataclass
class KmerFreqResult:
    """Every key of `poregen kmer_freq`: counts[code] for the 4^k ACGT k-mers (code = 2-bit bases, first base most significant, so
    code order is byte order), plus the keys holding any other byte, ascending in byte order, with their counts."""
    k: int
    counts: np.ndarray                      # uint64[4^k]
    odd_keys: List[bytes]
    odd_counts: np.ndarray                  # uint64[len(odd_keys)]

    def entries(self):
        """(key, count) for every key in byte order: the std::map the reference prints (src/kmer_freq.cpp:185-192)."""
        dense = [bytes(t) for t in itertools.product(b"ACGT", repeat=self.k)]
        out, j = [], 0
        for code, key in enumerate(dense):
            while j < len(self.odd_keys) and self.odd_keys[j] < key:
                out.append((self.odd_keys[j], int(self.odd_counts[j]))); j += 1
            out.append((key, int(self.counts[code])))
        out += [(self.odd_keys[i], int(self.odd_counts[i])) for i in range(j, len(self.odd_keys))]
        return out

    def lines(self, sort: int = 0, print_absent: int = 1) -> bytes:
        """The bytes `poregen kmer_freq --sort S --print_absent_kmers P` writes (src/kmer_freq.cpp:194-220)."""
        e = self.entries()
        if sort == 1:
            e.sort(key=lambda t: (t[1], t[0]))
        elif sort == 2:
            e.sort(key=lambda t: (t[1], t[0]), reverse=True)
        return b"".join(b"%s\t%d\n" % (key, c) for key, c in e if print_absent or c)


class KmerCounter:
    """Counts the k-mers of FASTQ bytes on the GPU (pg_kfreq_*). submit() takes the file's bytes in pieces cut anywhere: `bytes`,
    a numpy uint8 array, or a CUDA torch.uint8 tensor (read in place, no host copy; kept alive until finish). submit_fasta() takes a
    FASTA the same way, submit_reads() packed BAM reads; one stream (up to finish) takes one of the three."""

    def __init__(self, k: int, device: int = 0):
        self._lib = _abi.load()
        self.k = k
        h = C.c_void_p()
        st = self._lib.pg_kfreq_create(k, device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_kfreq_last_error(None).decode())
        self._h = h
        self._keep = []

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_kfreq_last_error(self._h).decode())

    def _submit_text(self, fn, piece):
        if hasattr(piece, "is_cuda") and piece.is_cuda:
            if piece.dtype.itemsize != 1 or not piece.is_contiguous():
                raise ValueError("device pieces must be contiguous uint8 tensors")
            self._keep.append(piece)
            self._check(fn(self._h, C.c_void_p(piece.data_ptr()), piece.numel(), _abi.PG_LOC_DEVICE))
            return
        a = np.ascontiguousarray(np.frombuffer(piece, np.uint8) if isinstance(piece, (bytes, bytearray, memoryview)) else piece, dtype=np.uint8)
        if a.size:
            self._check(fn(self._h, C.c_void_p(a.ctypes.data), a.size, _abi.PG_LOC_HOST))

    def submit(self, piece):
        self._submit_text(self._lib.pg_kfreq_submit, piece)

    def submit_fasta(self, piece):
        """The next bytes of a FASTA (pg_kfreq_submit_fasta): '>' lines are headers, a record's sequence is the lines between two of
        them joined, and its windows run across the line ends. Pieces as for submit()."""
        self._submit_text(self._lib.pg_kfreq_submit_fasta, piece)

    @property
    def reads_piece(self) -> int:
        """Window starts per piece of a long read in submit_reads (pg_kfreq_reads_piece)."""
        return int(self._lib.pg_kfreq_reads_piece(self._h))

    def submit_reads(self, seq_bytes, byte_off, l_seq, reverse, n_to_t: bool = False):
        """Layout rule: read r is l_seq[r] bases from byte byte_off[r] of seq_bytes, BAM's 4-bit codes "=ACMGRSVTWYHKDBN", high nibble first.
        seq_bytes uint8, byte_off uint64, l_seq uint32, reverse uint8 (non-zero: counted reverse-complemented): all four numpy arrays
        (`bytes` for seq_bytes too), or all four contiguous CUDA tensors of those widths (read in place, kept alive until finish).
        n_to_t counts N as T. A stream takes either submit() or submit_reads() until finish()."""
        flags = _abi.PG_KFREQ_N_TO_T if n_to_t else 0
        arrs = (seq_bytes, byte_off, l_seq, reverse)
        if all(hasattr(a, "is_cuda") and a.is_cuda for a in arrs):
            for a, size in zip(arrs, (1, 8, 4, 1)):
                if a.dtype.itemsize != size or not a.is_contiguous():
                    raise ValueError("device reads: contiguous tensors of 1-, 8-, 4- and 1-byte integers")
            n = l_seq.numel()
            if byte_off.numel() != n or reverse.numel() != n:
                raise ValueError("byte_off, l_seq and reverse must have one entry per read")
            self._keep.append(arrs)
            self._check(self._lib.pg_kfreq_submit_reads(self._h, C.c_void_p(seq_bytes.data_ptr()), seq_bytes.numel(), C.c_void_p(byte_off.data_ptr()),
                                                        C.c_void_p(l_seq.data_ptr()), C.c_void_p(reverse.data_ptr()), n, flags, _abi.PG_LOC_DEVICE))
            return
        if any(hasattr(a, "is_cuda") and a.is_cuda for a in arrs):
            raise ValueError("submit_reads takes four host arrays or four device tensors, not a mixture")
        s = np.ascontiguousarray(np.frombuffer(seq_bytes, np.uint8) if isinstance(seq_bytes, (bytes, bytearray, memoryview)) else seq_bytes, dtype=np.uint8)
        o = np.ascontiguousarray(byte_off, dtype=np.uint64)
        ln = np.ascontiguousarray(l_seq, dtype=np.uint32)
        rv = np.ascontiguousarray(reverse, dtype=np.uint8)
        if o.size != ln.size or rv.size != ln.size:
            raise ValueError("byte_off, l_seq and reverse must have one entry per read")
        self._check(self._lib.pg_kfreq_submit_reads(self._h, C.c_void_p(s.ctypes.data), s.size, C.c_void_p(o.ctypes.data), C.c_void_p(ln.ctypes.data),
                                                    C.c_void_p(rv.ctypes.data), ln.size, flags, _abi.PG_LOC_HOST))

    def finish(self) -> KmerFreqResult:
        counts = np.zeros(4 ** self.k, np.uint64)
        r = _abi.PgKfreqResult()
        try:
            self._check(self._lib.pg_kfreq_finish(self._h, C.c_void_p(counts.ctypes.data), C.byref(r)))
        finally:
            self._keep = []
        n = int(r.n_odd)
        raw = C.string_at(r.odd_keys, n * self.k) if n else b""
        keys = [raw[i * self.k:(i + 1) * self.k] for i in range(n)]
        oc = np.ctypeslib.as_array(C.cast(r.odd_counts, C.POINTER(C.c_uint64)), (n,)).copy() if n else np.zeros(0, np.uint64)
        return KmerFreqResult(self.k, counts, keys, oc)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_kfreq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmer_freq(data, k: int, device: int = 0, fasta: bool = False) -> KmerFreqResult:
    """One-shot: the k-mer counts of a whole FASTQ (fasta=True: a whole FASTA) given as bytes / numpy uint8 / CUDA uint8 tensor."""
    kc = KmerCounter(k, device)
    try:
        (kc.submit_fasta if fasta else kc.submit)(data)
        return kc.finish()
    finally:
        kc.close()


@dataclass
class F1Counts:
    """(TP, FP, TN, FN) over all pairs (`totals`) and per pair (`pairs`, n x 4), as f1score.py's compare_files sums them."""
    totals: np.ndarray
    pairs: np.ndarray


class AlignmentScorer:
    """Compares pairs of ss signal alignments on the GPU (pg_fscore_*), the per-point rules of the reference's f1score.py. submit() takes
    the ss strings of n pairs concatenated (string 2p = side 1, 2p + 1 = side 2 of pair p; `bytes`, numpy uint8, or a CUDA torch.uint8
    tensor read in place and kept alive until finish), 2n + 1 offsets, and per string the first signal index and first reference
    position (side 2 with base_shift already added). region = (start, end) applies f1score.py's --region point filter."""

    def __init__(self, rna: bool = False, threshold: int = 0, region=None, device: int = 0):
        self._lib = _abi.load()
        p = _abi.PgF1Params(int(bool(rna)), int(region is not None), int(threshold),
                            int(region[0]) if region is not None else 0, int(region[1]) if region is not None else 0)
        h = C.c_void_p()
        st = self._lib.pg_fscore_create(C.byref(p), device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_fscore_last_error(None).decode())
        self._h = h
        self._keep = []
        self._n = 0
        self.last_result = None

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_fscore_last_error(self._h).decode())

    def submit(self, ss, offsets, sig_start, first_ref):
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        sig = np.ascontiguousarray(sig_start, dtype=np.int64)
        ref = np.ascontiguousarray(first_ref, dtype=np.int64)
        ns = off.size - 1
        if ns < 0 or ns % 2 or sig.size != ns or ref.size != ns:
            raise ValueError("need 2n + 1 offsets and 2n start signals / first refs")
        if hasattr(ss, "is_cuda") and ss.is_cuda:
            if ss.dtype.itemsize != 1 or not ss.is_contiguous():
                raise ValueError("device ss must be a contiguous uint8 tensor")
            self._keep.append(ss)
            ptr, loc = ss.data_ptr(), _abi.PG_LOC_DEVICE
        else:
            a = np.ascontiguousarray(np.frombuffer(ss, np.uint8) if isinstance(ss, (bytes, bytearray, memoryview)) else ss, dtype=np.uint8)
            if ns and int(off[-1]) > a.size:
                raise ValueError("offsets run past the ss bytes")
            ptr, loc = (a.ctypes.data if a.size else None), _abi.PG_LOC_HOST
        b = _abi.PgF1Batch(ns // 2, loc, 0, ptr, off.ctypes.data, sig.ctypes.data, ref.ctypes.data)
        self._check(self._lib.pg_fscore_submit(self._h, C.byref(b)))
        self._n += ns // 2

    def finish(self) -> F1Counts:
        r = _abi.PgF1Result()
        n_cap = self._n
        pairs = np.zeros((max(n_cap, 1), 4), np.uint64)
        self._n = 0
        try:
            st = self._lib.pg_fscore_sync(self._h)
            self._check(st)
            st = self._lib.pg_fscore_finish(self._h, C.byref(r), C.c_void_p(pairs.ctypes.data), n_cap)
            self.last_result = r
            self._check(st)
        finally:
            self._keep = []
        n = int(r.n_pairs)
        return F1Counts(np.array(list(r.totals), np.uint64), pairs[:n].copy())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_fscore_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def f1_counts(ss, offsets, sig_start, first_ref, rna: bool = False, threshold: int = 0, region=None, device: int = 0) -> F1Counts:
    """One-shot AlignmentScorer: totals and per-pair (TP, FP, TN, FN)."""
    sc = AlignmentScorer(rna, threshold, region, device)
    try:
        sc.submit(ss, offsets, sig_start, first_ref)
        return sc.finish()
    finally:
        sc.close()


# ---- subtool0 / pa_stats ----------------------------------------------------------------------------------------------------------

@dataclass
class PaMeans:
    """`poregen subtool0` per read and `poregen pa_stats` per dataset: `means` (float64, NaN for a read without samples) print with "%f"
    exactly as the reference prints them; n_fallback reads were finished on the host by the reference's sequential loop; n_samples, mean
    and sstdev (sample standard deviation) are over every pA value."""
    means: np.ndarray
    n_fallback: int
    n_samples: int
    mean: float
    sstdev: float


class SignalMeans:
    """Mean pA of every read and of the dataset on the GPU (pg_pamean_*). submit() takes one batch in the pg_batch signal layout: int16
    samples, n + 1 offsets, and per read digitisation / offset / range -- numpy arrays, or CUDA torch tensors read in place (int64 offsets,
    float64 parameters; kept alive until finish). finish() returns every read since the last finish, in submission order."""

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        h = C.c_void_p()
        st = self._lib.pg_pamean_create(device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_pamean_last_error(None).decode())
        self._h = h
        self._keep = []
        self._means = []

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_pamean_last_error(self._h).decode())

    def submit(self, sig, sig_off, digitisation, offset, range):
        arrs = (sig, sig_off, digitisation, offset, range)
        dev = [hasattr(a, "is_cuda") and a.is_cuda for a in arrs]
        if any(dev):
            if not all(dev):
                raise ValueError("device input: all five arrays must be CUDA tensors")
            for a, itemsize in zip(arrs, (2, 8, 8, 8, 8)):
                if a.dtype.itemsize != itemsize or not a.is_contiguous():
                    raise ValueError("device input: contiguous int16 samples, 64-bit offsets, float64 parameters")
            n = sig_off.numel() - 1
            if n > 0 and int(sig_off[-1].item()) > sig.numel():  # (the kernels trust the offsets: never let them point past the samples)
                raise ValueError("sig_off runs past the samples")
            loc = _abi.PG_LOC_DEVICE
            kept = list(arrs)
        else:
            kept = [np.ascontiguousarray(sig, np.int16), np.ascontiguousarray(sig_off, np.uint64),
                    np.ascontiguousarray(digitisation, np.float64), np.ascontiguousarray(offset, np.float64),
                    np.ascontiguousarray(range, np.float64)]
            n = kept[1].size - 1
            if n > 0 and int(kept[1][-1]) > kept[0].size:
                raise ValueError("sig_off runs past the samples")
            loc = _abi.PG_LOC_HOST
        if n < 0 or any((a.numel() if hasattr(a, "numel") else a.size) != n for a in kept[2:]):
            raise ValueError("need n + 1 offsets and n digitisation / offset / range values")
        means = np.empty(max(n, 0), np.float64)
        b = _abi.PgPameanBatch(n, loc, 0, *[_ptr(a) if (hasattr(a, "numel") and a.numel()) or (isinstance(a, np.ndarray) and a.size) else None
                                             for a in kept])
        self._keep.append(kept)
        self._check(self._lib.pg_pamean_submit(self._h, C.byref(b), C.c_void_p(means.ctypes.data) if n else None))
        self._means.append(means)

    def submit_svb(self, blocks, block_off, digitisation, offset, range):
        """submit() for a batch whose samples are still svb-zd blocks (SignalDecoder): uint8 bytes in a numpy array or a CUDA tensor,
        n + 1 host offsets into them, host parameters. The blocks are decoded on the device; a corrupt block raises PgError
        (PG_ERR_INPUT) and nothing of the batch is counted."""
        blocks, boff, loc = _svb_arrays(blocks, block_off)
        par = [np.ascontiguousarray(a, np.float64) for a in (digitisation, offset, range)]
        n = boff.size - 1
        if any(a.size != n for a in par):
            raise ValueError("need n + 1 offsets and n digitisation / offset / range values")
        means = np.empty(n, np.float64)
        sb = _abi.PgSvbBatch(n, loc, 0, _ptr(blocks) if _size(blocks) else None, _size(blocks), boff.ctypes.data)
        self._check(self._lib.pg_pamean_submit_svb(self._h, C.byref(sb), *[C.c_void_p(a.ctypes.data) if n else None for a in par],
                                                    C.c_void_p(means.ctypes.data) if n else None))
        self._means.append(means)

    @property
    def svb_samples(self) -> int:
        """samples submit_svb has decoded on the device since this object was created"""
        return int(self._lib.pg_pamean_svb_samples(self._h))

    def finish(self) -> PaMeans:
        r = _abi.PgPameanResult()
        try:
            self._check(self._lib.pg_pamean_finish(self._h, C.byref(r)))
            means = np.concatenate(self._means) if self._means else np.zeros(0, np.float64)
        finally:
            self._keep, self._means = [], []
        return PaMeans(means, int(r.n_fallback), int(r.n_samples), float(r.mean), float(r.sstdev))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_pamean_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_means(sig, sig_off, digitisation, offset, range, device: int = 0) -> PaMeans:
    """One-shot SignalMeans: per-read means, the fallback count and the dataset summary of one batch (host or device arrays)."""
    sm = SignalMeans(device)
    try:
        sm.submit(sig, sig_off, digitisation, offset, range)
        return sm.finish()
    finally:
        sm.close()


def read_means_svb(blocks, block_off, digitisation, offset, range, device: int = 0) -> PaMeans:
    """read_means() for one batch of svb-zd blocks (SignalMeans.submit_svb)."""
    sm = SignalMeans(device)
    try:
        sm.submit_svb(blocks, block_off, digitisation, offset, range)
        return sm.finish()
    finally:
        sm.close()


# ---- svb-zd signal blocks (pg_sigdec_*) --------------------------------------------------------------------------------------------

def _size(a):
    return a.numel() if hasattr(a, "numel") else a.size


def _svb_arrays(blocks, block_off):
    """(blocks, block_off as uint64, location): blocks a contiguous uint8 numpy array or CUDA tensor, the offsets inside it"""
    if hasattr(blocks, "is_cuda") and blocks.is_cuda:
        if blocks.dtype.itemsize != 1 or not blocks.is_contiguous():
            raise ValueError("device blocks: a contiguous uint8 tensor")
        loc = _abi.PG_LOC_DEVICE
    else:
        blocks = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else blocks, np.uint8)
        loc = _abi.PG_LOC_HOST
    boff = np.ascontiguousarray(block_off, np.uint64)
    if boff.ndim != 1 or boff.size < 1:
        raise ValueError("need n + 1 block offsets")
    if (boff[1:] < boff[:-1]).any() or int(boff[-1]) > _size(blocks):  # (the kernels trust the offsets: never let them point past the bytes)
        raise ValueError("block_off decreases or runs past the blocks")
    return blocks, boff, loc


class SignalDecoder:
    """svb-zd signal blocks of BLOW5 records decoded on the GPU (pg_sigdec_*): read r's block is blocks[block_off[r]:block_off[r + 1]],
    bytes in a numpy array or a CUDA tensor, at any byte offset."""

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        h = C.c_void_p()
        st = self._lib.pg_sigdec_create(device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_sigdec_last_error(None).decode())
        self._h = h
        self._device = device

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_sigdec_last_error(self._h).decode())

    def counts(self, blocks, block_off) -> np.ndarray:
        """the samples each read decodes to (uint32): the block's count field, 0 for a block the host's checks refuse"""
        blocks, boff, loc = _svb_arrays(blocks, block_off)
        n = boff.size - 1
        out = np.zeros(n, np.uint32)
        self._check(self._lib.pg_sigdec_counts(self._h, _ptr(blocks) if _size(blocks) else None, _size(blocks), boff.ctypes.data, n, loc,
                                               out.ctypes.data if n else None))
        return out

    def decode(self, blocks, block_off, sig_off=None, out=None):
        """(samples, sig_off, bad): an int16 CUDA tensor with read r at [sig_off[r], sig_off[r] + count_r), the offsets (uint64) and the
        mask of corrupt blocks, whose spans hold unspecified samples. sig_off=None puts the reads back to back. out: the tensor to decode
        into (int16, contiguous, on the decoder's device, at least sig_off[-1] samples); nothing outside the spans is written."""
        import torch
        blocks, boff, loc = _svb_arrays(blocks, block_off)
        n = boff.size - 1
        if sig_off is None:
            cnt = self.counts(blocks, boff)
            soff = np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]).astype(np.uint64)
        else:
            soff = np.ascontiguousarray(sig_off, np.uint64)
            if soff.size != n + 1 or (soff[1:] < soff[:-1]).any():
                raise ValueError("need n + 1 non-decreasing sample offsets")
        total = int(soff[-1])
        if out is None:
            out = torch.empty(total, dtype=torch.int16, device=f"cuda:{self._device}")
        elif not (out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= total):
            raise ValueError("out: a contiguous int16 CUDA tensor of at least sig_off[-1] samples")
        bad = np.zeros(n, np.uint8)
        self._check(self._lib.pg_sigdec_decode(self._h, _ptr(blocks) if _size(blocks) else None, _size(blocks), boff.ctypes.data, n, loc,
                                               out.data_ptr() if out.numel() else None, soff.ctypes.data, bad.ctypes.data if n else None))
        return out, soff, bad.astype(bool)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_sigdec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_svb_zd(blocks, block_off, device: int = 0):
    """One-shot SignalDecoder: (samples, sig_off, bad) of one batch of svb-zd blocks, the reads back to back."""
    dec = SignalDecoder(device)
    try:
        return dec.decode(blocks, block_off)
    finally:
        dec.close()


class SignalEncoder:
    """int16 samples encoded into svb-zd signal blocks on the GPU (pg_sigenc_*), the shortest block of every read as slow5lib writes it:
    read r is sig[sig_off[r]:sig_off[r + 1]], samples in a numpy array or, read in place, in a CUDA tensor."""

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        h = C.c_void_p()
        st = self._lib.pg_sigenc_create(device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_sigenc_last_error(None).decode())
        self._h = h
        self._device = device

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_sigenc_last_error(self._h).decode())

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.pg_sigenc_set_stream(self._h, ptr))

    @property
    def stream(self) -> int:
        return int(self._lib.pg_sigenc_stream(self._h) or 0)

    def bound(self, sig_off) -> int:
        """no batch with these offsets encodes to more bytes (host only)"""
        soff = np.ascontiguousarray(sig_off, np.uint64)
        return int(self._lib.pg_sigenc_bound(soff.ctypes.data, max(soff.size - 1, 0)))

    def encode(self, sig, sig_off):
        """(blocks, block_off): a uint8 CUDA tensor that aliases the encoder's buffer (valid until its next encode / close) and the
        n + 1 block offsets (uint64, a copy). Both go to SignalDecoder.decode and SignalMeans.submit_svb as they are. The offsets are
        handed to the library as given: it refuses the ones that decrease, a read beyond 2^32 - 1 samples and more than 2^28 samples."""
        import torch
        soff = np.ascontiguousarray(sig_off, np.uint64)
        if soff.ndim != 1 or soff.size < 1:
            raise ValueError("need n + 1 sample offsets")
        n = soff.size - 1
        if hasattr(sig, "is_cuda") and sig.is_cuda:
            if sig.dtype != torch.int16 or not sig.is_contiguous():
                raise ValueError("device samples: a contiguous int16 tensor")
            loc = _abi.PG_LOC_DEVICE
        else:
            sig = np.ascontiguousarray(sig, np.int16)
            loc = _abi.PG_LOC_HOST
        if (soff[1:] >= soff[:-1]).all() and int(soff[-1]) > _size(sig) and int(soff[-1]) - int(soff[0]) <= (1 << 28):
            raise ValueError("sig_off runs past the samples")  # (the kernels trust the offsets: never let them point past the samples)
        res = _abi.PgSigencResult()
        res.struct_size = C.sizeof(_abi.PgSigencResult)
        self._check(self._lib.pg_sigenc_encode(self._h, _ptr(sig) if _size(sig) else None, soff.ctypes.data, n, loc, C.byref(res)))
        nb = int(res.n_block_bytes)
        boff = np.ctypeslib.as_array(C.cast(res.block_off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        dev = torch.device("cuda", self._device)
        if not nb:
            return torch.empty(0, dtype=torch.uint8, device=dev), boff

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            __cuda_array_interface__ = {"shape": (nb,), "typestr": "|u1", "data": (int(res.blocks), False), "version": 2}

        return torch.as_tensor(_Alias(), device=dev), boff

    def kernel_ms(self):
        """HIP-event time of the sizes kernel and of the emit kernel since the last call."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.pg_sigenc_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_sigenc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_svb_zd(sig, sig_off, device: int = 0):
    """One-shot SignalEncoder: (blocks, block_off) of one batch of reads; blocks is a CUDA tensor of its own."""
    enc = SignalEncoder(device)
    try:
        blocks, boff = enc.encode(sig, sig_off)
        return blocks.clone(), boff
    finally:
        enc.close()


# ---- model: the k-mer model from the text of dump files (pg_dmodel_*) ------------------------------------------------------------------

@dataclass
class DumpModelInfo:
    n_files: int
    n_bytes: int
    n_values: int          # values the device parsed
    n_host_files: int      # files finished on the host (outside the strict grammar, or declined by the reduction)
    host_files: np.ndarray
    n_batches: int
    parse_ms: float        # device time of the parse kernels / of the reduction (profile=True), else 0
    model_ms: float


def _model_arrays(m, text_of) -> "Model":
    ns = m.n_slots

    def arr(ptr, dt):
        if ns == 0 or not ptr:
            return np.zeros(0, dtype=dt)
        return np.frombuffer((C.c_char * (ns * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy()
    texts = [[text_of(s, which) for s in range(ns)] for which in (_abi.PG_MODEL_TEXT_MEDIAN, _abi.PG_MODEL_TEXT_SSTDEV, _abi.PG_MODEL_TEXT_DWELL)]
    return Model(n_values=arr(m.n_values, np.uint64), median=arr(m.median, np.float64), sstdev=arr(m.sstdev, np.float64),
                 mid_lo=arr(m.mid_lo, np.int64), mid_hi=arr(m.mid_hi, np.int64), origin=arr(m.origin, np.int64),
                 sum1=arr(m.sum1, np.int64), sum2_lo=arr(m.sum2_lo, np.uint64), sum2_hi=arr(m.sum2_hi, np.uint64),
                 dwell_n=arr(m.dwell_n, np.uint64), dwell_median=arr(m.dwell_median, np.float64),
                 median_text=texts[0], sstdev_text=texts[1], dwell_text=texts[2])


class DumpModel:
    """The k-mer model of dump FILES on the GPU (pg_dmodel_*): submit() takes a batch of files as one buffer of their bytes -- `bytes`, a
    numpy uint8 array, or a CUDA torch.uint8 tensor (read in place, kept alive until finish) -- and file_off[n_files + 1]; finish()
    returns a Model with one entry per file in submission order, and a DumpModelInfo."""

    def __init__(self, keep_first: bool = False, device: int = 0, profile: bool = False, events: bool = False, keep_events: bool = False):
        self._lib = _abi.load()
        h = C.c_void_p()
        flags = (_abi.PG_MODEL_KEEP_FIRST if keep_first else 0) | (_abi.PG_DMODEL_PROFILE if profile else 0)
        flags |= (_abi.PG_DMODEL_EVENTS if events or keep_events else 0) | (_abi.PG_DMODEL_EVENTS_KEEP if keep_events else 0)
        self._keep_events = keep_events
        st = self._lib.pg_dmodel_create(device, flags, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_dmodel_last_error(None).decode())
        self._h = h
        self._keep = []

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_dmodel_last_error(self._h).decode())

    def submit(self, data, file_off):
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("file_off needs n_files + 1 entries")
        if hasattr(data, "is_cuda") and data.is_cuda:
            if data.dtype.itemsize != 1 or not data.is_contiguous() or data.numel() < int(off[-1]):
                raise ValueError("device data must be a contiguous uint8 tensor of file_off[-1] bytes")
            self._keep.append(data)
            self._check(self._lib.pg_dmodel_submit(self._h, C.c_void_p(data.data_ptr()), C.c_void_p(off.ctypes.data), off.size - 1, _abi.PG_LOC_DEVICE))
            return
        a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
        if a.size < int(off[-1]):
            raise ValueError("data is shorter than file_off[-1]")
        self._check(self._lib.pg_dmodel_submit(self._h, C.c_void_p(a.ctypes.data) if a.size else None, C.c_void_p(off.ctypes.data), off.size - 1, _abi.PG_LOC_HOST))

    def finish(self):
        m = _abi.PgModelResult()
        info = _abi.PgDmodelInfo()
        try:
            self._check(self._lib.pg_dmodel_finish(self._h, C.byref(m), C.byref(info)))
        finally:
            self._keep = []
        buf = C.create_string_buffer(64)

        def text_of(s, which):
            n = self._lib.pg_dmodel_format(self._h, s, which, buf, 64)
            return buf.raw[:n].decode()
        nh = int(info.n_host_files)
        hf = np.ctypeslib.as_array(info.host_files, (nh,)).copy() if nh else np.zeros(0, np.uint32)
        return _model_arrays(m, text_of), DumpModelInfo(int(info.n_files), int(info.n_bytes), int(info.n_values), nh, hf, int(info.n_batches),
                                                        float(info.parse_ms), float(info.model_ms))

    def finish_events(self) -> "EventModel":
        """The event table of the files of the last finish() (DumpModel(events=True); finish() is called when it was not): an EventModel with
        one entry per file in submission order."""
        em, es = _abi.PgModelResult(), _abi.PgModelResult()
        st, ne = C.c_void_p(), C.c_void_p()
        self._check(self._lib.pg_dmodel_finish_events(self._h, C.byref(em), C.byref(es), C.byref(st), C.byref(ne)))
        self._keep = []
        nf = em.n_slots
        buf = C.create_string_buffer(64)

        def side(m, col0):
            def text_of(s, which):
                if which == _abi.PG_MODEL_TEXT_DWELL:
                    return ""
                n = self._lib.pg_dmodel_format_events(self._h, s, col0 + which, buf, 64)
                return buf.raw[:n].decode()
            return _model_arrays(m, text_of)
        status = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint32)), (nf,)).copy() if nf else np.zeros(0, np.uint32)
        n_events = np.ctypeslib.as_array(C.cast(ne, C.POINTER(C.c_uint64)), (nf,)).copy() if nf else np.zeros(0, np.uint64)
        ev_mean = ev_sd = None
        if self._keep_events:
            pm, ps, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
            if self._lib.pg_dmodel_events_values(self._h, C.byref(pm), C.byref(ps), C.byref(n)) != 0:
                raise PgError(-1, "pg_dmodel_events_values failed")
            take = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), (n.value,)).copy() if n.value else np.zeros(0, np.int64)
            ev_mean, ev_sd = take(pm), take(ps)
        a, b = C.c_double(0), C.c_double(0)
        self._lib.pg_dmodel_events_ms(self._h, C.byref(a), C.byref(b))
        return EventModel(means=side(em, _abi.PG_EVENTS_COL_MEAN_MEDIAN), sds=side(es, _abi.PG_EVENTS_COL_SD_MEDIAN), status=status, n_events=n_events,
                          refusal=[self._lib.pg_dmodel_events_refusal(self._h, f).decode() for f in range(nf)], ev_mean=ev_mean, ev_sd=ev_sd,
                          event_ms=a.value, reduce_ms=b.value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_dmodel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def list_dump_dirs(dirs):
    """(names, paths): the sorted union of the directories' file names (byte order; dot files and everything that is not a regular file
    skipped) and, per name, its files in argument order -- what `poregen model` reads."""
    import os
    found = {}
    for d in dirs:
        for name in os.listdir(os.fsencode(d)):
            path = os.path.join(os.fsencode(d), name)
            if not name.startswith(b".") and os.path.isfile(path):
                found.setdefault(name, []).append(path)
    names = sorted(found)
    return [os.fsdecode(n) for n in names], [found[n] for n in names]


def _submit_dump_files(dm, paths, batch_bytes):
    """the files of list_dump_dirs through dm.submit: batches of whole logical files (a name's files back to back), cut at batch_bytes"""
    chunks, off = [], [0]

    def flush():
        if len(off) > 1:
            dm.submit(b"".join(chunks), off)
        chunks.clear(); del off[1:]
    for ps in paths:
        data = b"".join(open(p, "rb").read() for p in ps)
        if len(off) > 1 and off[-1] + len(data) > batch_bytes:
            flush()
        chunks.append(data); off.append(off[-1] + len(data))
    flush()


def model_from_dumps(dirs, limit: str = "3.1", keep_first: bool = False, batch_bytes: int = 64 << 20, device: int = 0, profile: bool = False):
    """One-shot `poregen model`: (raw_lines, dwell_lines, info) of the dump directories -- NAME<TAB>median<TAB>stddev (capped at `limit`) and
    NAME<TAB>median dwell per file name; files of one name in several directories are read back to back."""
    if isinstance(dirs, (str, bytes)) or hasattr(dirs, "__fspath__"):
        dirs = [dirs]
    names, paths = list_dump_dirs(dirs)
    dm = DumpModel(keep_first=keep_first, device=device, profile=profile)
    try:
        _submit_dump_files(dm, paths, batch_bytes)
        m, info = dm.finish()
    finally:
        dm.close()
    return m.raw_model_lines(names, limit), m.dwell_lines(names), info


def event_model_from_dumps(dirs, keep_first: bool = False, batch_bytes: int = 64 << 20, device: int = 0, profile: bool = False, keep_events: bool = False):
    """One-shot `poregen model --event_model`: (names, EventModel, info) of the dump directories; EventModel.lines(names) is the table's
    text. keep_first only decides, in rare corners, which files `poregen model` finishes on the host (and whose table is refused for it)."""
    if isinstance(dirs, (str, bytes)) or hasattr(dirs, "__fspath__"):
        dirs = [dirs]
    names, paths = list_dump_dirs(dirs)
    dm = DumpModel(keep_first=keep_first, device=device, profile=profile, events=True, keep_events=keep_events)
    try:
        _submit_dump_files(dm, paths, batch_bytes)
        _, info = dm.finish()
        ev = dm.finish_events()
    finally:
        dm.close()
    return names, ev, info


@dataclass
class PoolResult:
    """pg_pool_finish: `model` has one entry per group, labeling after labeling (dwell fields 0 / NaN; a refused group reads as empty)."""
    model: "Model"
    status: np.ndarray        # per group: _abi.PG_POOL_GROUP_OK / _EMPTY / _REFUSED
    refused_file: np.ndarray  # per group: the first file (submission order) that caused the refusal, else -1
    n_files: np.ndarray       # per group: members
    refusal: list             # per group: the message, "" when not refused
    n_files_total: int
    n_bytes: int
    n_values: int             # values in the arena
    n_batches: int
    select_ms: float          # device time of the seven histogram passes


class DumpPool:
    """Median and sstdev of POOLS of dump files on the GPU (pg_pool_*): `n_groups[l]` groups in labeling l; submit() takes a batch of files
    as DumpModel.submit does plus group[l][file] (PG_POOL_NO_GROUP: in none); the files of a group count in submission order, as if
    concatenated. finish() returns a PoolResult. A group with a file the device path declines is refused: pools have no host path."""

    def __init__(self, n_groups, keep_first: bool = False, max_values: int = 0, device: int = 0):
        self._lib = _abi.load()
        ng = np.ascontiguousarray(n_groups, dtype=np.uint32).reshape(-1)
        h = C.c_void_p()
        st = self._lib.pg_pool_create(device, ng.size, C.c_void_p(ng.ctypes.data), int(max_values), _abi.PG_MODEL_KEEP_FIRST if keep_first else 0, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_pool_last_error(None).decode())
        self._h = h
        self.n_groups = [int(x) for x in ng]

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_pool_last_error(self._h).decode())

    def submit(self, data, file_off, group):
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("file_off needs n_files + 1 entries")
        g = np.ascontiguousarray(group, dtype=np.uint32).reshape(-1)
        if g.size != len(self.n_groups) * (off.size - 1):
            raise ValueError("group needs n_labelings * n_files entries")
        if hasattr(data, "is_cuda") and data.is_cuda:
            if data.dtype.itemsize != 1 or not data.is_contiguous() or data.numel() < int(off[-1]):
                raise ValueError("device data must be a contiguous uint8 tensor of file_off[-1] bytes")
            self._check(self._lib.pg_pool_submit(self._h, C.c_void_p(data.data_ptr()), C.c_void_p(off.ctypes.data), off.size - 1, C.c_void_p(g.ctypes.data), _abi.PG_LOC_DEVICE))
            return
        a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
        if a.size < int(off[-1]):
            raise ValueError("data is shorter than file_off[-1]")
        self._check(self._lib.pg_pool_submit(self._h, C.c_void_p(a.ctypes.data) if a.size else None, C.c_void_p(off.ctypes.data), off.size - 1,
                                             C.c_void_p(g.ctypes.data), _abi.PG_LOC_HOST))

    def finish(self) -> PoolResult:
        r = _abi.PgPoolResult()
        self._check(self._lib.pg_pool_finish(self._h, C.byref(r)))
        buf = C.create_string_buffer(64)
        ng = int(r.n_groups)

        def text_of(s, which):
            if which == _abi.PG_MODEL_TEXT_DWELL:
                return ""
            n = self._lib.pg_pool_format(self._h, s, which, buf, 64)
            return buf.raw[:n].decode()

        def arr(ptr, dt):
            return np.frombuffer((C.c_char * (ng * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy() if ng and ptr else np.zeros(0, dt)
        return PoolResult(model=_model_arrays(r.model, text_of), status=arr(r.status, np.uint32), refused_file=arr(r.refused_file, np.int64),
                          n_files=arr(r.n_files, np.uint64), refusal=[self._lib.pg_pool_refusal(self._h, g).decode() for g in range(ng)],
                          n_files_total=int(r.n_files_total), n_bytes=int(r.n_bytes), n_values=int(r.n_values), n_batches=int(r.n_batches),
                          select_ms=float(r.select_ms))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_pool_names(names):
    """(K, alphabet) of dump file names that can be pooled: one length, all over ACGT or all over ACGU. ValueError names the first offender."""
    if not names:
        raise ValueError("no dump files")
    k = len(names[0])
    for n in names:
        if len(n) != k:
            raise ValueError(f"{n}: the names have more than one length ({len(n)} against {k})")
    alphabet = None
    for n in names:
        for c in n:
            if c not in "ACGTU":
                raise ValueError(f"{n}: a name that is no k-mer over ACGT or ACGU")
            if c in "TU":
                if alphabet is None:
                    alphabet = c
                elif alphabet != c:
                    raise ValueError(f"{n}: the names mix T and U")
    return k, "ACG" + (alphabet or "T")


def _pool_run(dirs, groups_of, n_groups, keep_first, batch_bytes, device, max_values):
    names, paths = list_dump_dirs(dirs)
    pool = DumpPool(n_groups, keep_first=keep_first, max_values=max_values, device=device)
    try:
        chunks, off, gids = [], [0], []

        def flush():
            if len(off) > 1:
                pool.submit(b"".join(chunks), off, np.array(gids, np.uint32).T)
            chunks.clear(); del off[1:]; gids.clear()
        for name, ps in zip(names, paths):
            data = b"".join(open(p, "rb").read() for p in ps)
            if len(off) > 1 and off[-1] + len(data) > batch_bytes:
                flush()
            chunks.append(data); off.append(off[-1] + len(data)); gids.append(groups_of(name))
        flush()
        res = pool.finish()
    finally:
        pool.close()
    for g in range(len(res.status)):
        if res.status[g] == _abi.PG_POOL_GROUP_REFUSED:
            raise PgError(_abi.PG_ERR_UNSUPPORTED, f"group {g} is refused: {names[int(res.refused_file[g])]}: {res.refusal[g]}")
    return names, res


def _as_dirs(dirs):
    return [dirs] if isinstance(dirs, (str, bytes)) or hasattr(dirs, "__fspath__") else list(dirs)


def pool_from_dumps(dirs, start: int, length: int, limit: str = "3.1", keep_first: bool = False, batch_bytes: int = 64 << 20, device: int = 0, max_values: int = 0):
    """One-shot `poregen model --pool START:LEN`: (lines, PoolResult) -- SUB<TAB>median<TAB>stddev (capped at `limit`) for every sub-k-mer
    name[start:start + length] that occurs, its files pooled in the byte order of their names."""
    dirs = _as_dirs(dirs)
    names, _ = list_dump_dirs(dirs)
    k, _ = check_pool_names(names)
    if start < 0 or length < 1 or start + length > k:
        raise ValueError(f"--pool {start}:{length} does not lie inside names of length {k}")
    subs = sorted({n[start:start + length] for n in names}, key=lambda x: x.encode())
    index = {sub: i for i, sub in enumerate(subs)}
    names, res = _pool_run(dirs, lambda n: [index[n[start:start + length]]], [len(subs)], keep_first, batch_bytes, device, max_values)
    return res.model.raw_model_lines(subs, limit), res


def offsets_from_dumps(dirs, keep_first: bool = False, batch_bytes: int = 64 << 20, device: int = 0, max_values: int = 0):
    """One-shot `poregen offsets`: (text, PoolResult) -- the `base`, `spread` and `best` rows the command prints, tab-separated."""
    dirs = _as_dirs(dirs)
    names, _ = list_dump_dirs(dirs)
    k, alphabet = check_pool_names(names)
    if k > _abi.PG_POOL_MAX_LABELINGS:
        raise ValueError(f"names of length {k}: offsets takes k-mers of at most {_abi.PG_POOL_MAX_LABELINGS} bases")
    names, res = _pool_run(dirs, lambda n: [alphabet.index(c) for c in n], [4] * k, keep_first, batch_bytes, device, max_values)
    m = res.model
    lines, spreads = [], []
    for pos in range(k):
        halves = []
        for b in range(4):
            g = 4 * pos + b
            nv = int(m.n_values[g])
            lines.append("\t".join(["base", str(pos), alphabet[b], str(int(res.n_files[g])), str(nv), m.median_text[g], m.sstdev_text[g]]))
            if nv:
                halves.append(int(m.mid_lo[g]) + int(m.mid_hi[g]))
        spreads.append(max(halves) - min(halves) if len(halves) >= 2 else None)
    for pos, sp in enumerate(spreads):
        lines.append("\t".join(["spread", str(pos), "" if sp is None else _half_units_text(sp)]))
    if any(sp is not None for sp in spreads):
        lines.append("best\t%d" % max((pos for pos, sp in enumerate(spreads) if sp is not None), key=lambda p: (spreads[p], -p)))
    return "".join(l + "\n" for l in lines), res


def _half_units_text(s: int) -> str:
    """"%.14Lg" of s / (2 * 10^8) in long double (s an integer of half units): its 14 significant digits, printed as %g prints them"""
    from decimal import Decimal
    x = np.longdouble(s) / np.longdouble(200000000)
    if x == 0:
        return "0"
    mant, exp = np.format_float_scientific(x, precision=13, unique=False, exp_digits=2).split("e")
    return "%.14g" % float(Decimal(mant).scaleb(int(exp)))


def transform_model(raw_text, stdv, mean, stdv_min="2.5", stdv_max="4", stdv_from=None) -> str:
    """`poregen transform` (STEP 7, scripts/poregen.sh:87-148): the final model file from a raw model's KMER<TAB>median<TAB>stddev rows.
    level_mean' = (level_mean * stdv) + mean and level_stdv projected onto [stdv_min, stdv_max], digit for digit as `bc -l` prints them; the
    four constants are decimal TEXTS (a float would lose the digits bc keeps). stdv_from: the text of another model file whose level_stdv
    column replaces the projected one, row by row. Host only: no GPU is touched. ValueError with the library's message when the model is
    refused (a field that is no number to bc, a k-mer without samples, max == min, ...)."""
    def enc(x):
        return x if isinstance(x, bytes) else str(x).encode()
    lib = _abi.load()
    raw = enc(raw_text)
    frm = None if stdv_from is None else enc(stdv_from)
    out, n_out, err = C.c_void_p(), C.c_size_t(), C.create_string_buffer(512)
    st = lib.pg_transform_model(raw, len(raw), enc(stdv), enc(mean), enc(stdv_min), enc(stdv_max), frm, 0 if frm is None else len(frm),
                                C.byref(out), C.byref(n_out), err, len(err))
    if st != _abi.PG_OK:
        raise ValueError(err.value.decode(errors="replace"))
    try:
        return C.string_at(out, n_out.value).decode()
    finally:
        lib.pg_transform_free(out)


# ---- move tables to ss ops (pg_mvops_*) ------------------------------------------------------------------------------------------------

class MoveOps:
    """The result of MoveExpander.expand: CUDA tensors that alias the expander's device buffers (valid until its next expand / close), in
    the layout of a pg_batch -- op_n uint32 (as int32 bits), op_t uint8, op_off int64[n + 1], query_start / target_start / target_end
    int32[n], seq uint8 (ASCII), seq_off int64[n + 1], status int32[n] -- plus n_ops, n_refused, first_refused and the statuses on the
    host (numpy uint32[n])."""

    def __init__(self, res, device):
        import torch

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        dev = torch.device("cuda", device)

        def wrap(ptr, n, typestr, dtype):
            if n == 0 or not ptr:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_Alias(ptr, n, typestr), device=dev)

        n = int(res.n_reads)
        self.n_reads, self.n_ops, self.n_seq = n, int(res.n_ops), int(res.n_seq)
        self.n_refused, self.first_refused = int(res.n_refused), int(res.first_refused)
        self.op_n = wrap(res.op_n, self.n_ops, "<i4", torch.int32)
        self.op_t = wrap(res.op_t, self.n_ops, "|u1", torch.uint8)
        self.op_off = wrap(res.op_off, n + 1, "<i8", torch.int64)
        self.query_start = wrap(res.query_start, n, "<i4", torch.int32)
        self.target_start = wrap(res.target_start, n, "<i4", torch.int32)
        self.target_end = wrap(res.target_end, n, "<i4", torch.int32)
        self.seq = wrap(res.seq, self.n_seq, "|u1", torch.uint8)
        self.seq_off = wrap(res.seq_off, n + 1, "<i8", torch.int64)
        self.status_device = wrap(res.status, n, "<i4", torch.int32)
        self.status = np.ctypeslib.as_array(C.cast(res.status_host, C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)

    def to_host(self):
        """Every array as numpy, in the widths of the ABI (op_n uint32, offsets uint64)."""
        return dict(op_n=self.op_n.cpu().numpy().view(np.uint32), op_t=self.op_t.cpu().numpy(), op_off=self.op_off.cpu().numpy().view(np.uint64),
                    query_start=self.query_start.cpu().numpy(), target_start=self.target_start.cpu().numpy(), target_end=self.target_end.cpu().numpy(),
                    seq=self.seq.cpu().numpy(), seq_off=self.seq_off.cpu().numpy().view(np.uint64), status=self.status_device.cpu().numpy().view(np.uint32))


class RefOps:
    """The result of MoveExpander.project: CUDA tensors that alias the expander's device buffers (valid until its next project / close), in
    the layout of a pg_batch -- op_n uint32 (as int32 bits), op_t uint8, op_off int64[n + 1], query_start / target_start / target_end /
    query_end int32[n], ref_len / n_match / status int32[n] -- plus n_ops, n_refused, first_refused and, on the host (numpy), status,
    ref_len, n_match (uint32[n]) and query_end (int32[n])."""

    def __init__(self, res, device):
        import torch

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        dev = torch.device("cuda", device)

        def wrap(ptr, n, typestr, dtype):
            if n == 0 or not ptr:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_Alias(ptr, n, typestr), device=dev)

        def host(ptr, ctype, dtype):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).copy() if n else np.zeros(0, dtype)

        n = int(res.n_reads)
        self.n_reads, self.n_ops = n, int(res.n_ops)
        self.n_refused, self.first_refused = int(res.n_refused), int(res.first_refused)
        self.op_n = wrap(res.op_n, self.n_ops, "<i4", torch.int32)
        self.op_t = wrap(res.op_t, self.n_ops, "|u1", torch.uint8)
        self.op_off = wrap(res.op_off, n + 1, "<i8", torch.int64)
        for name in ("query_start", "target_start", "target_end", "query_end", "ref_len", "n_match"):
            setattr(self, name, wrap(getattr(res, name), n, "<i4", torch.int32))
        self.status_device = wrap(res.status, n, "<i4", torch.int32)
        self.status = host(res.status_host, C.c_uint32, np.uint32)
        self.ref_len_host = host(res.ref_len_host, C.c_uint32, np.uint32)
        self.n_match_host = host(res.n_match_host, C.c_uint32, np.uint32)
        self.query_end_host = host(res.query_end_host, C.c_int32, np.int32)

    def to_host(self):
        """Every device array as numpy, in the widths of the ABI (op_n, ref_len, n_match, status uint32, op_off uint64)."""
        out = dict(op_n=self.op_n.cpu().numpy().view(np.uint32), op_t=self.op_t.cpu().numpy(), op_off=self.op_off.cpu().numpy().view(np.uint64),
                   status=self.status_device.cpu().numpy().view(np.uint32))
        for name in ("query_start", "target_start", "target_end", "query_end"):
            out[name] = getattr(self, name).cpu().numpy()
        for name in ("ref_len", "n_match"):
            out[name] = getattr(self, name).cpu().numpy().view(np.uint32)
        return out


class MoveExpander:
    """Expands the move tables of a batch of BAM records into the ss ops `poregen reform -c -k 1 -m 0` prints (pg_mvops_*). The nine
    arrays of expand() are numpy arrays, or contiguous CUDA tensors of the same widths (read in place)."""

    _ARGS = (("mv", 1, np.int8), ("mv_off", 8, np.uint64), ("stride", 4, np.int32), ("ns", 8, np.uint64), ("ts", 8, np.uint64), ("l_seq", 4, np.uint32),
             ("flag", 4, np.uint32), ("seq_bytes", 1, np.uint8), ("byte_off", 8, np.uint64))

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        self.device = device
        h = C.c_void_p()
        st = self._lib.pg_mvops_create(device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_mvops_last_error(None).decode())
        self._h = h

    @property
    def piece(self) -> int:
        """Table elements per piece of a long read (pg_mvops_piece)."""
        return int(self._lib.pg_mvops_piece(self._h))

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the expander's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        st = self._lib.pg_mvops_set_stream(self._h, ptr)
        if st != 0:
            raise PgError(st, self._lib.pg_mvops_last_error(self._h).decode())

    def expand(self, mv, mv_off, stride, ns, ts, l_seq, flag, seq_bytes, byte_off, rna: bool = False, n_to_t: bool = False) -> MoveOps:
        given = (mv, mv_off, stride, ns, ts, l_seq, flag, seq_bytes, byte_off)
        on_dev = [hasattr(a, "is_cuda") and a.is_cuda for a in given]
        b = _abi.PgMvopsBatch()
        b.flags = (_abi.PG_MVOPS_RNA if rna else 0) | (_abi.PG_MVOPS_N_TO_T if n_to_t else 0)
        if all(on_dev):
            for a, (name, size, _) in zip(given, self._ARGS):
                if a.dtype.itemsize != size or not a.is_contiguous():
                    raise ValueError(f"device batch: {name} must be a contiguous tensor of {size}-byte integers")
            keep = given
            ptrs = [C.c_void_p(a.data_ptr()) for a in given]
            sizes = [a.numel() for a in given]
            b.location = _abi.PG_LOC_DEVICE
        elif any(on_dev):
            raise ValueError("expand takes nine host arrays or nine device tensors, not a mixture")
        else:
            keep = [np.ascontiguousarray(np.frombuffer(a, dt) if isinstance(a, (bytes, bytearray, memoryview)) else a, dtype=dt) for a, (_, _, dt) in zip(given, self._ARGS)]
            ptrs = [C.c_void_p(a.ctypes.data) for a in keep]
            sizes = [a.size for a in keep]
            b.location = _abi.PG_LOC_HOST
        n = sizes[5]
        if sizes[1] != n + 1 or any(sizes[i] != n for i in (2, 3, 4, 6, 8)):
            raise ValueError("mv_off needs n + 1 entries; stride, ns, ts, l_seq, flag and byte_off one per read")
        b.n_reads = n
        b.mv, b.mv_off, b.stride, b.ns, b.ts, b.l_seq, b.flag, b.seq_bytes, b.byte_off = ptrs
        b.n_mv_bytes, b.n_seq_bytes = sizes[0], sizes[7]
        res = _abi.PgMvopsResult()
        st = self._lib.pg_mvops_expand(self._h, C.byref(b), C.byref(res))
        del keep
        if st != 0:
            raise PgError(st, self._lib.pg_mvops_last_error(self._h).decode())
        return MoveOps(res, self.device)

    def project(self, ops, cigar, cigar_off, pos, rna: bool = False, reverse=None, contig_len=None) -> RefOps:
        """Carries ops through the records' CIGARs onto the reference (pg_mvops_project). ops: a MoveOps (read in place), or a tuple of
        CUDA tensors (op_n, op_off, query_start, status) of 4, 8, 4 and 4-byte integers. cigar (uint32 words len << 4 | op), cigar_off
        (uint64[n + 1]) and pos (int32[n], 0-based) are three numpy arrays or three contiguous CUDA tensors of the same widths.
        reverse (uint8[n], non-zero: a reverse-strand record) and contig_len (int32[n]), given together and lying where the CIGAR arrays
        lie, make it pg_mvops_project_stranded: a reverse read is placed on the reverse complement of its contig."""
        if (reverse is None) != (contig_len is None):
            raise ValueError("project: reverse and contig_len go together")
        op_n, op_off, qs, status = (ops.op_n, ops.op_off, ops.query_start, ops.status_device) if isinstance(ops, MoveOps) else ops
        for a, size, name in ((op_n, 4, "op_n"), (op_off, 8, "op_off"), (qs, 4, "query_start"), (status, 4, "status")):
            if not (hasattr(a, "is_cuda") and a.is_cuda) or a.dtype.itemsize != size or not a.is_contiguous():
                raise ValueError(f"project: {name} must be a contiguous CUDA tensor of {size}-byte integers")
        n = op_off.numel() - 1
        if n < 0 or qs.numel() != n or status.numel() != n:
            raise ValueError("project: op_off needs n + 1 entries, query_start and status one per read")
        given = (cigar, cigar_off, pos) + (() if reverse is None else (reverse, contig_len))
        widths = (("cigar", 4, np.uint32), ("cigar_off", 8, np.uint64), ("pos", 4, np.int32), ("reverse", 1, np.uint8), ("contig_len", 4, np.int32))
        on_dev = [hasattr(a, "is_cuda") and a.is_cuda for a in given]
        c = _abi.PgMvopsCigars()
        if all(on_dev):
            for a, (name, size, _) in zip(given, widths):
                if a.dtype.itemsize != size or not a.is_contiguous():
                    raise ValueError(f"device CIGARs: {name} must be a contiguous tensor of {size}-byte integers")
            keep = given
            ptrs = [C.c_void_p(a.data_ptr()) if a.numel() else None for a in given]
            sizes = [a.numel() for a in given]
            c.location = _abi.PG_LOC_DEVICE
        elif any(on_dev):
            raise ValueError("project takes host arrays or device tensors of CIGARs (and strands), not a mixture")
        else:
            keep = [np.ascontiguousarray(a, dtype=dt) for a, (_, _, dt) in zip(given, widths)]
            ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in keep]
            sizes = [a.size for a in keep]
            c.location = _abi.PG_LOC_HOST
        if sizes[1] != n + 1 or any(x != n for x in sizes[2:]):
            raise ValueError("project: cigar_off needs n + 1 entries, pos (reverse, contig_len) one per read")
        c.n_reads, c.flags = n, (_abi.PG_MVOPS_RNA if rna else 0)
        c.op_n, c.n_ops, c.op_off = (C.c_void_p(op_n.data_ptr()) if op_n.numel() else None), op_n.numel(), C.c_void_p(op_off.data_ptr())
        c.query_start, c.status = (C.c_void_p(qs.data_ptr()) if n else None), (C.c_void_p(status.data_ptr()) if n else None)
        c.cigar, c.cigar_off, c.pos = ptrs[:3]
        c.n_cigar = sizes[0]
        res = _abi.PgMvopsProjection()
        if reverse is None:
            st = self._lib.pg_mvops_project(self._h, C.byref(c), C.byref(res))
        else:
            strands = _abi.PgMvopsStrands()
            strands.reverse, strands.contig_len = ptrs[3:]
            st = self._lib.pg_mvops_project_stranded(self._h, C.byref(c), C.byref(strands), C.byref(res))
        del keep
        if st != 0:
            raise PgError(st, self._lib.pg_mvops_last_error(self._h).decode())
        return RefOps(res, self.device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_mvops_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reform_ops(mv, mv_off, stride, ns, ts, l_seq, flag, seq_bytes, byte_off, rna: bool = False, n_to_t: bool = False, device: int = 0):
    """One-shot MoveExpander.expand: the result's arrays on the host (MoveOps.to_host) plus n_ops, n_refused and first_refused."""
    ex = MoveExpander(device)
    try:
        r = ex.expand(mv, mv_off, stride, ns, ts, l_seq, flag, seq_bytes, byte_off, rna=rna, n_to_t=n_to_t)
        out = r.to_host()
        out.update(n_ops=r.n_ops, n_refused=r.n_refused, first_refused=r.first_refused)
        return out
    finally:
        ex.close()


def project_ops(op_n, op_off, query_start, status, cigar, cigar_off, pos, rna: bool = False, device: int = 0, reverse=None, contig_len=None):
    """One-shot MoveExpander.project of host arrays (op_n uint32, op_off uint64[n + 1], query_start int32[n], status uint32[n], the
    CIGAR arrays and, for records of either strand, reverse and contig_len): the result's arrays on the host (RefOps.to_host) plus n_ops,
    n_refused and first_refused."""
    import torch
    ex = MoveExpander(device)
    try:
        dev = torch.device("cuda", device)
        up = [torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(vt)).to(dev)
              for a, dt, vt in ((op_n, np.uint32, np.int32), (op_off, np.uint64, np.int64), (query_start, np.int32, np.int32), (status, np.uint32, np.int32))]
        r = ex.project(tuple(up), cigar, cigar_off, pos, rna=rna, reverse=reverse, contig_len=contig_len)
        out = r.to_host()
        out.update(n_ops=r.n_ops, n_refused=r.n_refused, first_refused=r.first_refused)
        return out
    finally:
        ex.close()


# ---- refseq: the reference slices of mapped reads, gathered on the device (pg_refseq_*) ------------------------------------------------

class RefSlices:
    """The result of RefSeq.slices: seq (uint8) and seq_off (int64[n + 1]) as CUDA tensors that alias the handle's device buffers (valid
    until its next slices / close), laid out as a pg_batch takes them, and n_seq."""

    def __init__(self, res, n, device):
        import torch

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        dev = torch.device("cuda", device)
        self.n_reads, self.n_seq = int(n), int(res.n_seq)
        self.seq = torch.as_tensor(_Alias(res.seq, self.n_seq, "|u1"), device=dev) if self.n_seq else torch.empty(0, dtype=torch.uint8, device=dev)
        self.seq_off = torch.as_tensor(_Alias(res.seq_off, n + 1, "<i8"), device=dev)

    def to_host(self):
        """[bytes] per read."""
        seq, off = self.seq.cpu().numpy().tobytes(), self.seq_off.cpu().numpy()
        return [seq[int(off[r]):int(off[r + 1])] for r in range(self.n_reads)]


class RefSeq:
    """Reference contigs on the device, added one by one, and the slices mapped reads take of them (pg_refseq_*): what `gmove --reform
    --ref` fetches per read, reversed and complemented for a reverse-strand read."""

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        self.device = device
        h = C.c_void_p()
        st = self._lib.pg_refseq_create(device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_refseq_last_error(None).decode())
        self._h = h

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        st = self._lib.pg_refseq_set_stream(self._h, ptr)
        if st != 0:
            raise PgError(st, self._lib.pg_refseq_last_error(self._h).decode())

    def add(self, bases) -> int:
        """A contig's bases (bytes, line ends removed); returns the index reads name it by."""
        b = bytes(bases)
        idx = C.c_int32(-1)
        st = self._lib.pg_refseq_add(self._h, C.cast(C.c_char_p(b), C.c_void_p) if b else None, len(b), C.byref(idx))
        if st != 0:
            raise PgError(st, self._lib.pg_refseq_last_error(self._h).decode())
        return int(idx.value)

    def slices(self, contig, pos, ref_len, reverse=None) -> RefSlices:
        """contig (int32[n], -1: no such contig), pos (int32[n]), ref_len (uint32[n]) and reverse (uint8[n] or None): numpy arrays, or
        contiguous CUDA tensors of the same widths."""
        given = (contig, pos, ref_len) + (() if reverse is None else (reverse,))
        widths = (("contig", 4, np.int32), ("pos", 4, np.int32), ("ref_len", 4, np.uint32), ("reverse", 1, np.uint8))
        on_dev = [hasattr(a, "is_cuda") and a.is_cuda for a in given]
        rd = _abi.PgRefseqReads()
        if all(on_dev):
            for a, (name, size, _) in zip(given, widths):
                if a.dtype.itemsize != size or not a.is_contiguous():
                    raise ValueError(f"device reads: {name} must be a contiguous tensor of {size}-byte integers")
            keep = given
            ptrs = [C.c_void_p(a.data_ptr()) if a.numel() else None for a in given]
            sizes = [a.numel() for a in given]
            rd.location = _abi.PG_LOC_DEVICE
        elif any(on_dev):
            raise ValueError("slices takes host arrays or device tensors, not a mixture")
        else:
            keep = [np.ascontiguousarray(a, dtype=dt) for a, (_, _, dt) in zip(given, widths)]
            ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in keep]
            sizes = [a.size for a in keep]
            rd.location = _abi.PG_LOC_HOST
        n = sizes[0]
        if any(x != n for x in sizes):
            raise ValueError("slices: contig, pos, ref_len (and reverse) hold one entry per read")
        rd.n_reads = n
        rd.contig, rd.pos, rd.ref_len = ptrs[:3]
        rd.reverse = ptrs[3] if reverse is not None else None
        res = _abi.PgRefseqSlices()
        st = self._lib.pg_refseq_slice(self._h, C.byref(rd), C.byref(res))
        del keep
        if st != 0:
            raise PgError(st, self._lib.pg_refseq_last_error(self._h).decode())
        return RefSlices(res, n, self.device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_refseq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ref_slices(contigs, contig, pos, ref_len, reverse=None, device: int = 0):
    """One-shot RefSeq: contigs (a list of bytes) go up in order, so `contig` indexes the list; returns the slices as a list of bytes."""
    rs = RefSeq(device)
    try:
        for c in contigs:
            rs.add(c)
        return rs.slices(contig, pos, ref_len, reverse).to_host()
    finally:
        rs.close()


# ---- fit: a k-mer model scored against signal and move tables (pg_fit_*) --------------------------------------------------------------

FIT_STATUS_NAMES = {0: "ok", 1: "out_of_signal", 2: "too_long", 3: "few_events", 4: "flat", 5: "negative_scale", 6: "ref_length",
                    17: "no_move_in_table", 18: "negative_tail", 19: "bases_left_over", 20: "bad_stride"}


def units_text(v: int) -> str:
    """An integer of 1e-3 pA with three decimals, as the k-mer table prints it."""
    v = int(v)
    return f"{'-' if v < 0 else ''}{abs(v) // 1000}.{abs(v) % 1000:03d}"


def parse_fit_model(text, k: int = 0):
    """(k, levels uint32[4^k] in 1e-3 pA with 0 for a missing k-mer, uses_u) of a model file in the format `poregen transform` writes
    (pg_fit_parse_model; no GPU needed). PgError with PG_ERR_INPUT when the model is refused."""
    lib = _abi.load()
    data = text.encode() if isinstance(text, str) else bytes(text)
    levels = np.zeros(4 ** 9, np.uint32)
    kk, uu, err = C.c_uint32(), C.c_int32(), C.create_string_buffer(400)
    st = lib.pg_fit_parse_model(data, len(data), k, C.byref(kk), levels.ctypes.data, levels.size, C.byref(uu), err, len(err))
    if st != 0:
        raise PgError(st, err.value.decode())
    return int(kk.value), levels[:4 ** kk.value].copy(), bool(uu.value)


@dataclass
class FitReads:
    """One submit: per read the seven sums (int64[n, 7]: N, SL, SLL, SR, SRL, SRR, E), the status and the fit sample = a + b * level."""
    sums: np.ndarray
    status: np.ndarray
    a: np.ndarray
    b: np.ndarray


@dataclass
class FitResult:
    """Everything since the last finish: per slot (k-mer rank in ACGT order) samples, events, sum d and sum d^2 (Python ints), the totals."""
    kmer_size: int
    n_samples: np.ndarray
    n_events: np.ndarray
    sum_d: np.ndarray
    sum_dd: list
    reads: int
    fitted: int
    events: int
    samples: int
    clamped: int

    def residuals(self, slot: int):
        """(mean_resid, rms_resid) of a slot in 1e-3 pA, None when it has no sample (pg_fit_residuals)."""
        n = int(self.n_samples[slot])
        if not n:
            return None
        return _fit_residuals(n, int(self.sum_d[slot]), self.sum_dd[slot])

    def pooled_rms(self):
        return _fit_residuals(self.samples, 0, sum(self.sum_dd))[1] if self.samples else None

    def kmer_table(self, levels, uses_u: bool = False) -> str:
        rows = []
        for s, kmer in enumerate(generate_kmers(self.kmer_size, rna=uses_u)):
            r = self.residuals(s)
            rows.append("\t".join([kmer, str(int(self.n_samples[s])), str(int(self.n_events[s])), units_text(levels[s]) if levels[s] else "",
                                   units_text(r[0]) if r else "", units_text(r[1]) if r else ""]) + "\n")
        return "".join(rows)


def _fit_residuals(n, sum_d, sum_dd):
    lib = _abi.load()
    m, q = C.c_int64(), C.c_int64()
    st = lib.pg_fit_residuals(n, sum_d, sum_dd & 0xffffffffffffffff, sum_dd >> 64, C.byref(m), C.byref(q))
    if st != 0:
        raise PgError(st, "pg_fit_residuals: sums out of range")
    return int(m.value), int(q.value)


class ReadScaling:
    """What ModelFit.calibrate leaves on the device for a batch of n_reads reads: sums (int64[n, 7]), status (int32, PG_FIT_ST_*), a, b,
    center, spread (float64) and use (uint8) as CUDA tensors; n_ok reads have use set, n_status[s] reads have status s (index 7: a skip
    code); solve_ms is the HIP-event time of the solve."""

    def __init__(self, res, device):
        import torch

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        dev = torch.device("cuda", device)
        n = self.n_reads = int(res.n_reads)
        self.n_ok, self.n_status, self.solve_ms = int(res.n_ok), [int(v) for v in res.n_status], float(res.solve_ms)

        def view(ptr, shape, typestr, dtype):
            return torch.as_tensor(_Alias(ptr, shape, typestr), device=dev) if n else torch.empty(shape, dtype=dtype, device=dev)
        self.sums = view(res.d_sums, (n, 7), "<i8", torch.int64)
        self.status = view(res.d_status, (n,), "<i4", torch.int32)
        self.a, self.b = view(res.d_a, (n,), "<f8", torch.float64), view(res.d_b, (n,), "<f8", torch.float64)
        self.center, self.spread = view(res.d_center, (n,), "<f8", torch.float64), view(res.d_spread, (n,), "<f8", torch.float64)
        self.use = view(res.d_use, (n,), "|u1", torch.uint8)


class ModelFit:
    """Scores a k-mer model against batches laid out as MoveExpander leaves them (pg_fit_*): submit() fits every read, finish() returns the
    per-k-mer residual sums. levels: uint32[4^k] in 1e-3 pA, 0 for a k-mer without a level."""

    def __init__(self, levels, k: int, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, min_events: int = 20, device: int = 0):
        self._lib = _abi.load()
        self.device, self._h = device, None
        p = _abi.PgFitParams(C.sizeof(_abi.PgFitParams), sig_move_offset, min_dur, max_dur, min_events, int(rna))
        h = C.c_void_p()
        st = self._lib.pg_fit_create(C.byref(p), device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_fit_last_error(None).decode())
        self._h = h
        self.set_model(levels, k)

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_fit_last_error(self._h).decode())

    def set_model(self, levels, k: int):
        lv = np.ascontiguousarray(levels, dtype=np.uint32)
        if lv.size != 4 ** k:
            raise ValueError("levels needs 4^k entries")
        self._check(self._lib.pg_fit_set_model(self._h, lv.ctypes.data, k))
        self.kmer_size = k

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.pg_fit_set_stream(self._h, ptr))

    def submit(self, batch: "Batch", skip=None) -> FitReads:
        """One batch (host or device) with all_matches set: the caller vouches that it holds match ops only, the device verifies it; or
        with gapped set: ops on the signal-to-reference alignment (I and D among them) and seq the reads' reference slices. A batch with
        neither flag, or with both, is refused (PG_ERR_INVALID_ARG). skip: per read a code, non-zero = the read takes no part."""
        cb = _c_batch(batch)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint32)
        out = _abi.PgFitReads()
        self._check(self._lib.pg_fit_submit(self._h, C.byref(cb), None if sk is None else sk.ctypes.data, C.byref(out)))
        n = int(out.n_reads)

        def arr(ptr, count, dt):
            if not count or not ptr:
                return np.zeros(0, dt)
            return np.frombuffer((C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy()
        return FitReads(sums=arr(out.sums, 7 * n, np.int64).reshape(n, 7), status=arr(out.status, n, np.uint32), a=arr(out.a, n, np.float64), b=arr(out.b, n, np.float64))

    def calibrate(self, batch: "Batch", skip=None) -> "ReadScaling":
        """One batch as submit() takes it, put on the model's pA scale (pg_fit_calibrate): pass 1, then the solve on the device and per
        read center = (a + offset) * g, spread = (b * 1000) * g with g = range / digitisation, use = the fit is ok and both are usable.
        Runs no pass 2 and adds nothing to finish(). The result's tensors alias the handle's device buffers (valid until its next
        submit / calibrate / close); GmoveEngine(scaling=2).submit(batch, scaling=...) takes it."""
        cb = _c_batch(batch)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint32)
        out = _abi.PgFitScaling()
        self._check(self._lib.pg_fit_calibrate(self._h, C.byref(cb), None if sk is None else sk.ctypes.data, C.byref(out)))
        return ReadScaling(out, self.device)

    def finish(self) -> FitResult:
        r = _abi.PgFitResult()
        self._check(self._lib.pg_fit_finish(self._h, C.byref(r)))
        ns = int(r.n_slots)

        def arr(ptr, dt):
            return np.frombuffer((C.c_char * (ns * 8)).from_address(ptr), dtype=dt).copy()
        lo, hi = arr(r.sum_dd_lo, np.uint64), arr(r.sum_dd_hi, np.uint64)
        return FitResult(kmer_size=int(r.kmer_size), n_samples=arr(r.n_samples, np.uint64), n_events=arr(r.n_events, np.uint64), sum_d=arr(r.sum_d, np.int64),
                         sum_dd=[(int(h) << 64) | int(l) for l, h in zip(lo, hi)], reads=int(r.reads), fitted=int(r.fitted), events=int(r.events),
                         samples=int(r.samples), clamped=int(r.clamped))

    def pass_ms(self):
        """HIP-event time of pass 1 and of pass 2 since the last call."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.pg_fit_pass_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_fit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_model(model_text, batches, k: int = 0, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, min_events: int = 20, device: int = 0):
    """One-shot: parse the model, submit every batch, finish. Returns ([FitReads per batch], FitResult, levels, uses_u)."""
    kk, levels, uses_u = parse_fit_model(model_text, k)
    mf = ModelFit(levels, kk, sig_move_offset=sig_move_offset, rna=rna, min_dur=min_dur, max_dur=max_dur, min_events=min_events, device=device)
    try:
        reads = [mf.submit(b) for b in batches]
        return reads, mf.finish(), levels, uses_u
    finally:
        mf.close()


# ---- realign: the move table's boundaries refined against a k-mer model (pg_realign_*) ---------------------------------------------------

@dataclass
class RealignReads:
    """One submit: op_n, the refined ops laid out as the batch's op_n (a torch uint32-as-int32 CUDA tensor; to_host() gives numpy uint32),
    and per read n_free, n_moved, sum_abs_shift (numpy) and cost_before / cost_after (lists of Python ints, 128 bits)."""
    op_n: object
    n_free: np.ndarray
    n_moved: np.ndarray
    sum_abs_shift: np.ndarray
    cost_before: list
    cost_after: list

    def to_host(self) -> np.ndarray:
        return self.op_n.cpu().numpy().view(np.uint32)


def _realign_params(sig_move_offset, rna, min_dur, max_dur, band, min_len, phase=0):
    return _abi.PgRealignParams(C.sizeof(_abi.PgRealignParams), sig_move_offset, min_dur, max_dur, int(rna), band, min_len, phase)


class Realigner:
    """Refines the ops of batches laid out as MoveExpander leaves them against a k-mer model (pg_realign_*). submit(batch, fit_reads) takes
    the FitReads that ModelFit.submit returned for the same batch under the same model and parameters; only the reads it fitted move.
    phase (0 .. 255): the boundaries e with e % 256 == phase are the pinned ones."""

    def __init__(self, levels, k: int, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, band: int = 10, min_len: int = 3, device: int = 0,
                 phase: int = 0):
        self._lib = _abi.load()
        self.device, self._h = device, None
        p = _realign_params(sig_move_offset, rna, min_dur, max_dur, band, min_len, phase)
        h = C.c_void_p()
        st = self._lib.pg_realign_create(C.byref(p), device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_realign_last_error(None).decode())
        self._h = h
        lv = np.ascontiguousarray(levels, dtype=np.uint32)
        if lv.size != 4 ** k:
            raise ValueError("levels needs 4^k entries")
        self._check(self._lib.pg_realign_set_model(self._h, lv.ctypes.data, k))
        self.kmer_size = k

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_realign_last_error(self._h).decode())

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.pg_realign_set_stream(self._h, ptr))

    def set_phase(self, phase: int):
        """The pinned period's phase for the following submits (rounds alternate 0 and 128)."""
        self._check(self._lib.pg_realign_set_phase(self._h, phase))

    def submit(self, batch: "Batch", fit_reads, copy: bool = True) -> RealignReads:
        """copy=False: op_n aliases the handle's own array, which stays valid until the submit after the next one -- a batch whose op_n it
        is may be submitted again (rounds)."""
        import torch
        cb = _c_batch(batch)
        st = np.ascontiguousarray(fit_reads.status, dtype=np.uint32)
        a = np.ascontiguousarray(fit_reads.a, dtype=np.float64)
        b = np.ascontiguousarray(fit_reads.b, dtype=np.float64)
        if not (st.size == a.size == b.size == batch.n_reads):
            raise ValueError("fit_reads is of another batch")
        out = _abi.PgRealignReads()
        out.struct_size = C.sizeof(_abi.PgRealignReads)
        self._check(self._lib.pg_realign_submit(self._h, C.byref(cb), st.ctypes.data, a.ctypes.data, b.ctypes.data, C.byref(out)))
        n, n_ops = int(out.n_reads), int(out.n_ops)
        rd = np.frombuffer((C.c_char * (n * C.sizeof(_abi.PgRealignRead))).from_address(out.reads), dtype=np.uint64).reshape(n, 6).copy() if n else np.zeros((0, 6), np.uint64)
        dev = torch.device("cuda", self.device)
        if n_ops:  # the handle's buffer lives until its next submit: the caller gets a copy (the submit is complete, the clone synchronised)
            class _Alias:
                __cuda_array_interface__ = {"shape": (n_ops,), "typestr": "<i4", "data": (int(out.op_n), False), "version": 2}
            op = torch.as_tensor(_Alias(), device=dev)
            if copy:
                op = op.clone()
                torch.cuda.current_stream(dev).synchronize()
        else:
            op = torch.empty(0, dtype=torch.int32, device=dev)
        return RealignReads(op_n=op, n_free=(rd[:, 0] & 0xffffffff).astype(np.uint32), n_moved=(rd[:, 0] >> 32).astype(np.uint32), sum_abs_shift=rd[:, 1].copy(),
                            cost_before=[(int(h) << 64) | int(l) for l, h in zip(rd[:, 2], rd[:, 3])], cost_after=[(int(h) << 64) | int(l) for l, h in zip(rd[:, 4], rd[:, 5])])

    def kernel_ms(self) -> float:
        """HIP-event time of the alignment kernel since the last call."""
        ms = C.c_double()
        self._check(self._lib.pg_realign_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_realign_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def realign_ops(levels, k: int, batch: "Batch", fit_reads, **kw):
    """One-shot Realigner.submit: (refined ops as numpy uint32, RealignReads)."""
    with Realigner(levels, k, **kw) as ra:
        r = ra.submit(batch, fit_reads)
        return r.to_host(), r


def realign_rounds(levels, k: int, batch: "Batch", rounds: int, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, min_events: int = 20,
                   band: int = 10, min_len: int = 3, device: int = 0):
    """`rounds` (1 .. 8) rounds of fit and realign over one batch: round t fits ops_{t-1} (ops_0: the batch's), and refines them with that
    fit at phase 0 when t is odd, 128 when it is even; a read that is not fitted in a round keeps its ops in it. Returns (ops_R as numpy
    uint32, [RealignReads of every round], [FitReads of every round]). The batch is put on the device and left as it was handed in."""
    import copy as _copy
    if not 1 <= rounds <= 8:
        raise ValueError("rounds: 1 to 8")
    b = _copy.copy(batch if batch.on_device else batch.to_device(f"cuda:{device}"))
    fit = ModelFit(levels, k, sig_move_offset=sig_move_offset, rna=rna, min_dur=min_dur, max_dur=max_dur, min_events=min_events, device=device)
    try:
        with Realigner(levels, k, sig_move_offset=sig_move_offset, rna=rna, min_dur=min_dur, max_dur=max_dur, band=band, min_len=min_len, device=device) as ra:
            per_round, fits = [], []
            for t in range(1, rounds + 1):
                fr = fit.submit(b)
                fit.finish()
                ra.set_phase(0 if t % 2 else 128)
                got = ra.submit(b, fr, copy=False)
                b.op_n = got.op_n
                per_round.append(got); fits.append(fr)
            ops = per_round[-1].to_host().copy()
            for got in per_round:                                          # (the handle's arrays go with it)
                got.op_n = None
            return ops, per_round, fits
    finally:
        fit.close()


def realign_walk(levels, k: int, seq, ops, q: int, sig, a: float, b: float, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, band: int = 10,
                 min_len: int = 3, phase: int = 0, op_t=None):
    """The rule for one fitted read on the host (pg_realign_walk; no GPU needed): (refined ops, n_free, n_moved, sum_abs_shift, cost_before,
    cost_after), or None when the ops leave the samples. op_t: the read is a gapped one (seq its reference slice; pg_realign_walk_gapped),
    None as well when the slice has not as many bases as the ops have columns."""
    lib = _abi.load()
    p = _realign_params(sig_move_offset, rna, min_dur, max_dur, band, min_len, phase)
    lv = np.ascontiguousarray(levels, dtype=np.uint32)
    s = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)
    o = np.ascontiguousarray(ops, dtype=np.uint32)
    sg = np.ascontiguousarray(sig, dtype=np.int16)
    new = np.zeros(o.size, np.uint32)
    rd = _abi.PgRealignRead()
    if op_t is None:
        st = lib.pg_realign_walk(C.byref(p), lv.ctypes.data, k, s.ctypes.data, o.size, o.ctypes.data, q, sg.ctypes.data, sg.size, a, b, new.ctypes.data, C.byref(rd))
    else:
        t = np.ascontiguousarray(op_t, dtype=np.uint8)
        if t.size != o.size:
            raise ValueError("op_t needs one code per op")
        st = lib.pg_realign_walk_gapped(C.byref(p), lv.ctypes.data, k, s.ctypes.data, s.size, o.ctypes.data, t.ctypes.data, o.size, q, sg.ctypes.data, sg.size, a, b,
                                        new.ctypes.data, C.byref(rd))
    if st == _abi.PG_ERR_INPUT:
        return None
    if st != 0:
        raise PgError(st, "pg_realign_walk: bad argument")
    return new, rd.n_free, rd.n_moved, rd.sum_abs_shift, (rd.cost_before_hi << 64) | rd.cost_before_lo, (rd.cost_after_hi << 64) | rd.cost_after_lo


# ---- eventalign: one row per counted event against the k-mer model (pg_evalign_*) ----------------------------------------------------------

EVALIGN_HEADER = ("contig\tposition\treference_kmer\tread_index\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tmodel_kmer\tmodel_mean\tmodel_stdv\t"
                  "standardized_level\tstart_idx\tend_idx\n")


@dataclass
class EventRows:
    """One submit: row_off (uint64[n_reads + 1]), rows (a structured numpy array: read, event, start, n, slot, first, mean_u, stdv_u, z_c;
    ordered by (read, event)) and the text as bytes (None when the handle produces none)."""
    row_off: np.ndarray
    rows: np.ndarray
    text: Optional[bytes]


@dataclass
class EventMeta:
    """What the text says of every read beyond its rows: ref_start (int64), reverse (bool), contigs and labels (lists of str or bytes). Any
    of them None: 0, forward, empty, the decimal index of the read in the batch."""
    ref_start: object = None
    reverse: object = None
    contigs: object = None
    labels: object = None


def _evalign_params(sig_move_offset, rna, min_dur, max_dur, sample_rate, flags):
    return _abi.PgEvalignParams(C.sizeof(_abi.PgEvalignParams), sig_move_offset, min_dur, max_dur, int(rna), sample_rate, flags)


def _string_table(strings):
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(s) for s in raw])
    return np.frombuffer(b"".join(raw) or b"\0", np.uint8), off


class EventAligner:
    """The per-event table of batches laid out as MoveExpander leaves them against a k-mer model (pg_evalign_*). submit(batch, fit_reads)
    takes the FitReads that ModelFit.submit returned for the same batch under the same model and parameters; only the reads it fitted have
    rows. levels, stdvs: uint32[4^k] in 1e-3 pA; a k-mer with a level needs a stdv above 0 (PgError with PG_ERR_INPUT)."""

    def __init__(self, levels, stdvs, k: int, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, sample_rate: int = 0, text: bool = True,
                 device: int = 0):
        self._lib = _abi.load()
        self.device, self._h = device, None
        p = _evalign_params(sig_move_offset, rna, min_dur, max_dur, sample_rate, _abi.PG_EVALIGN_HOST_ROWS | (_abi.PG_EVALIGN_TEXT if text else 0))
        h = C.c_void_p()
        st = self._lib.pg_evalign_create(C.byref(p), device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_evalign_last_error(None).decode())
        self._h = h
        self.set_model(levels, stdvs, k)

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_evalign_last_error(self._h).decode())

    def set_model(self, levels, stdvs, k: int):
        lv, sd = np.ascontiguousarray(levels, dtype=np.uint32), np.ascontiguousarray(stdvs, dtype=np.uint32)
        if lv.size != 4 ** k or sd.size != 4 ** k:
            raise ValueError("levels and stdvs need 4^k entries")
        self._check(self._lib.pg_evalign_set_model(self._h, lv.ctypes.data, sd.ctypes.data, k))
        self.kmer_size = k

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.pg_evalign_set_stream(self._h, ptr))

    def submit(self, batch: "Batch", fit_reads, meta: Optional[EventMeta] = None) -> EventRows:
        cb = _c_batch(batch)
        st = np.ascontiguousarray(fit_reads.status, dtype=np.uint32)
        a = np.ascontiguousarray(fit_reads.a, dtype=np.float64)
        b = np.ascontiguousarray(fit_reads.b, dtype=np.float64)
        n = batch.n_reads
        if not (st.size == a.size == b.size == n):
            raise ValueError("fit_reads is of another batch")
        cm, keep = None, []
        if meta is not None:
            cm = _abi.PgEvalignMeta()
            if meta.ref_start is not None:
                rs = np.ascontiguousarray(meta.ref_start, dtype=np.int64); keep.append(rs); cm.ref_start = rs.ctypes.data
            if meta.reverse is not None:
                rv = np.ascontiguousarray(meta.reverse, dtype=np.uint8); keep.append(rv); cm.reverse = rv.ctypes.data
            for name, strings in (("contig", meta.contigs), ("label", meta.labels)):
                if strings is not None:
                    data, off = _string_table(strings); keep += [data, off]
                    setattr(cm, name, data.ctypes.data); setattr(cm, name + "_off", off.ctypes.data)
            for arr, name in ((meta.ref_start, "ref_start"), (meta.reverse, "reverse"), (meta.contigs, "contigs"), (meta.labels, "labels")):
                if arr is not None and len(arr) != n:
                    raise ValueError(f"meta.{name} needs one entry per read")
        out = _abi.PgEvalignOut()
        out.struct_size = C.sizeof(_abi.PgEvalignOut)
        self._check(self._lib.pg_evalign_submit(self._h, C.byref(cb), st.ctypes.data, a.ctypes.data, b.ctypes.data, None if cm is None else C.byref(cm), C.byref(out)))
        n_rows = int(out.n_rows)
        row_off = np.frombuffer((C.c_char * ((n + 1) * 8)).from_address(out.row_off), dtype=np.uint64).copy()
        rows = (np.frombuffer((C.c_char * (n_rows * 40)).from_address(out.rows_host), dtype=_abi.EVALIGN_ROW_DTYPE).copy() if n_rows
                else np.zeros(0, _abi.EVALIGN_ROW_DTYPE))
        text = None
        if out.text_bytes:
            buf = C.create_string_buffer(int(out.text_bytes))
            self._check(self._lib.pg_evalign_copy_text(self._h, buf, int(out.text_bytes)))
            text = buf.raw
        return EventRows(row_off=row_off, rows=rows, text=text)

    def kernel_ms(self):
        """HIP-event time of the three stages (count, rows, text) since the last call."""
        ms = (C.c_double * 3)()
        self._check(self._lib.pg_evalign_kernel_ms(self._h, ms))
        return tuple(ms)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_evalign_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def event_align(levels, stdvs, k: int, batch: "Batch", meta: Optional[EventMeta] = None, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70,
                min_events: int = 20, sample_rate: int = 0, device: int = 0):
    """One call: fit the batch, then its per-event table. Returns (FitReads, EventRows)."""
    fit = ModelFit(levels, k, sig_move_offset=sig_move_offset, rna=rna, min_dur=min_dur, max_dur=max_dur, min_events=min_events, device=device)
    try:
        fr = fit.submit(batch)
        with EventAligner(levels, stdvs, k, sig_move_offset=sig_move_offset, rna=rna, min_dur=min_dur, max_dur=max_dur, sample_rate=sample_rate, device=device) as ea:
            return fr, ea.submit(batch, fr, meta)
    finally:
        fit.close()


def eventalign_walk(levels, stdvs, k: int, seq, ops, q: int, sig, a: float, b: float, sig_move_offset: int = 0, rna: bool = False, min_dur: int = 5, max_dur: int = 70, op_t=None):
    """The rule for one fitted read on the host (pg_evalign_walk; no GPU needed): its rows as a structured numpy array (`read` 0), or None
    when the read has no fit's place (the ops leave the samples; gapped: the slice has not as many bases as the ops have columns). op_t:
    the read is a gapped one (seq its reference slice; pg_evalign_walk_gapped)."""
    lib = _abi.load()
    p = _evalign_params(sig_move_offset, rna, min_dur, max_dur, 0, 0)
    lv, sd = np.ascontiguousarray(levels, dtype=np.uint32), np.ascontiguousarray(stdvs, dtype=np.uint32)
    s = np.frombuffer((seq.encode() if isinstance(seq, str) else bytes(seq)) or b"\0", np.uint8)
    n_seq = len(seq)
    o = np.ascontiguousarray(ops, dtype=np.uint32)
    sg = np.ascontiguousarray(sig, dtype=np.int16)
    rows = np.zeros(max(o.size, 1), _abi.EVALIGN_ROW_DTYPE)
    nr = C.c_uint64()
    if op_t is None:
        st = lib.pg_evalign_walk(C.byref(p), lv.ctypes.data, sd.ctypes.data, k, s.ctypes.data, o.size, o.ctypes.data, q, sg.ctypes.data, sg.size, a, b, rows.ctypes.data, rows.size,
                                 C.byref(nr))
    else:
        t = np.ascontiguousarray(op_t, dtype=np.uint8)
        if t.size != o.size:
            raise ValueError("op_t needs one code per op")
        st = lib.pg_evalign_walk_gapped(C.byref(p), lv.ctypes.data, sd.ctypes.data, k, s.ctypes.data, n_seq, o.ctypes.data, t.ctypes.data, o.size, q, sg.ctypes.data, sg.size, a, b,
                                        rows.ctypes.data, rows.size, C.byref(nr))
    if st == _abi.PG_ERR_INPUT:
        return None
    if st != 0:
        raise PgError(st, "pg_evalign_walk: bad argument")
    return rows[:int(nr.value)].copy()


def eventalign_row_text(row, contig, label, kmer, n_seq: int, ref_start: int, reverse: bool, sample_rate: int, level: int, stdv: int) -> bytes:
    """The line of one row as the device writes it (pg_evalign_row_text; no GPU needed). kmer: the k letters of the read's seq at row.first."""
    lib = _abi.load()
    r = np.zeros(1, _abi.EVALIGN_ROW_DTYPE); r[0] = row
    c, lb, km = [x.encode() if isinstance(x, str) else bytes(x) for x in (contig, label, kmer)]
    buf = C.create_string_buffer(len(c) + len(lb) + 4096)
    n = lib.pg_evalign_row_text(r.ctypes.data, c, len(c), lb, len(lb), km, len(km), n_seq, ref_start, int(reverse), sample_rate, level, stdv, buf, len(buf))
    return buf.raw[:n]


# ---- simulate: raw signal and its true alignment drawn from a k-mer model (pg_sim_*) --------------------------------------------------------

SIM_STATUS_NAMES = {0: "ok", 1: "too_short", 2: "bad_base", 3: "no_level"}


def parse_sim_model(text, k: int = 0):
    """(k, levels, stdvs, uses_u) of a model file: parse_fit_model with the level_stdv column kept, uint32[4^k] in 1e-3 pA
    (pg_sim_parse_model; no GPU needed). PgError with PG_ERR_INPUT when the model is refused."""
    lib = _abi.load()
    data = text.encode() if isinstance(text, str) else bytes(text)
    levels, stdvs = np.zeros(4 ** 9, np.uint32), np.zeros(4 ** 9, np.uint32)
    kk, uu, err = C.c_uint32(), C.c_int32(), C.create_string_buffer(400)
    st = lib.pg_sim_parse_model(data, len(data), k, C.byref(kk), levels.ctypes.data, stdvs.ctypes.data, levels.size, C.byref(uu), err, len(err))
    if st != 0:
        raise PgError(st, err.value.decode())
    return int(kk.value), levels[:4 ** kk.value].copy(), stdvs[:4 ** kk.value].copy(), bool(uu.value)


def parse_dwell_model(text, k: int = 0):
    """(k, dwells uint32[4^k]) of the file `poregen model --dwell_model` writes, a median of x.5 rounded up, 0 for a k-mer the file does
    not give (pg_sim_parse_dwell; no GPU needed)."""
    lib = _abi.load()
    data = text.encode() if isinstance(text, str) else bytes(text)
    dw = np.zeros(4 ** 9, np.uint32)
    kk, err = C.c_uint32(), C.create_string_buffer(400)
    st = lib.pg_sim_parse_dwell(data, len(data), k, C.byref(kk), dw.ctypes.data, dw.size, err, len(err))
    if st != 0:
        raise PgError(st, err.value.decode())
    return int(kk.value), dw[:4 ** kk.value].copy()


def scale_stdvs(stdvs, noise_q8: int):
    """stdv <- (stdv * noise_q8 + 128) >> 8: the noise scale in 1 / 256, applied before the tables go to the simulator."""
    return ((np.asarray(stdvs, np.uint64) * np.uint64(noise_q8) + np.uint64(128)) >> np.uint64(8)).astype(np.uint32)


def _sim_params(k, sig_move_offset, rna, seed, digitisation, range_e4, offset, off_spread, spread_pct, lead, lead_level, lead_stdv):
    return _abi.PgSimParams(C.sizeof(_abi.PgSimParams), k, sig_move_offset, int(rna), seed, range_e4, digitisation, offset, off_spread, spread_pct, lead, lead_level, lead_stdv, 0)


def _sim_seq_arrays(seqs):
    data = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(data) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in data], dtype=np.uint64)
    return np.frombuffer(b"".join(data), np.uint8).copy(), off


@dataclass
class SimReads:
    """One generate: torch CUDA tensors that alias the simulator's device buffers (valid until its next generate / close), `batch`, a
    device Batch over them that ModelFit, Realigner and GmoveEngine take in place (all_matches), and the statuses on the host."""
    batch: "Batch"
    status: np.ndarray
    status_device: object
    n_ops: int
    n_samples: int
    n_refused: int

    def to_host(self):
        b = self.batch
        return dict(sig=b.sig.cpu().numpy()[:self.n_samples], sig_off=b.sig_off.cpu().numpy().view(np.uint64), digitisation=b.digitisation.cpu().numpy(),
                    offset=b.offset.cpu().numpy(), range=b.range.cpu().numpy(), query_start=b.query_start.cpu().numpy(), target_start=b.target_start.cpu().numpy(),
                    target_end=b.target_end.cpu().numpy(), seq=b.seq.cpu().numpy(), seq_off=b.seq_off.cpu().numpy().view(np.uint64),
                    op_n=b.op_n.cpu().numpy().view(np.uint32), op_t=b.op_t.cpu().numpy(), op_off=b.op_off.cpu().numpy().view(np.uint64), status=self.status.copy(),
                    status_device=self.status_device.cpu().numpy().view(np.uint32))


class SignalSimulator:
    """Draws raw signal and the ops that are true by construction from a k-mer model (pg_sim_*). levels, stdvs, dwells: uint32[4^k], the
    first two in 1e-3 pA (a level of 0: the k-mer has none), dwells in samples; range_e4 is the range in 1e-4 pA."""

    def __init__(self, levels, stdvs, dwells, k: int, sig_move_offset: int = 0, rna: bool = False, seed: int = 0, digitisation: int = 8192, range_e4: int = 14676100,
                 offset: int = 10, off_spread: int = 0, spread_pct: int = 50, lead: int = 0, lead_level=None, lead_stdv=None, device: int = 0):
        self._lib = _abi.load()
        self.device, self._h = device, None
        lv, sd, dw = (np.ascontiguousarray(a, dtype=np.uint32) for a in (levels, stdvs, dwells))
        if not (lv.size == sd.size == dw.size == 4 ** k):
            raise ValueError("levels, stdvs and dwells need 4^k entries each")
        have = lv[lv > 0]
        if lead_level is None:  # the rounded means of the model's columns
            lead_level = int((int(have.sum()) * 2 + have.size) // (2 * have.size)) if have.size else 0
        if lead_stdv is None:
            lead_stdv = int((int(sd[lv > 0].sum()) * 2 + have.size) // (2 * have.size)) if have.size else 0
        self.params = _sim_params(k, sig_move_offset, rna, seed, digitisation, range_e4, offset, off_spread, spread_pct, lead, lead_level, lead_stdv)
        h = C.c_void_p()
        st = self._lib.pg_sim_create(C.byref(self.params), device, C.byref(h))
        if st != 0:
            raise PgError(st, self._lib.pg_sim_last_error(None).decode())
        self._h = h
        self._check(self._lib.pg_sim_set_model(self._h, lv.ctypes.data, sd.ctypes.data, dw.ctypes.data, k))
        self.kmer_size = k

    def _check(self, st):
        if st != 0:
            raise PgError(st, self._lib.pg_sim_last_error(self._h).decode())

    def set_stream(self, stream=None):
        """Run on a caller-owned stream (a torch.cuda.Stream or a raw hipStream_t value); None: the handle's own."""
        ptr = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.pg_sim_set_stream(self._h, ptr))

    @property
    def stream(self) -> int:
        return int(self._lib.pg_sim_stream(self._h) or 0)

    def generate(self, seqs=None, first_read: int = 0, seq=None, seq_off=None) -> SimReads:
        """seqs: a list of str / bytes; or seq (uint8) and seq_off (n + 1 offsets) as numpy arrays or as CUDA tensors (uint8, int64)."""
        import torch
        if seqs is not None:
            seq, seq_off = _sim_seq_arrays(seqs)
        b = _abi.PgSimBatch()
        b.struct_size = C.sizeof(_abi.PgSimBatch)
        on_dev = hasattr(seq_off, "is_cuda") and seq_off.is_cuda
        if on_dev:
            if not (seq.is_cuda and seq.is_contiguous() and seq_off.is_contiguous() and seq.dtype.itemsize == 1 and seq_off.dtype.itemsize == 8):
                raise ValueError("device batch: seq must be a contiguous uint8 tensor and seq_off a contiguous int64 tensor")
            keep = (seq, seq_off)
            b.location, b.n_reads, b.seq, b.seq_off = _abi.PG_LOC_DEVICE, seq_off.numel() - 1, seq.data_ptr(), seq_off.data_ptr()
        else:
            keep = (np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(seq_off, dtype=np.uint64))
            b.location, b.n_reads, b.seq, b.seq_off = _abi.PG_LOC_HOST, keep[1].size - 1, keep[0].ctypes.data, keep[1].ctypes.data
        b.first_read = first_read
        res = _abi.PgSimResult()
        res.struct_size = C.sizeof(_abi.PgSimResult)
        self._check(self._lib.pg_sim_generate(self._h, C.byref(b), C.byref(res)))
        dev = torch.device("cuda", self.device)

        class _Alias:  # zero-copy hand-over through the CUDA array interface
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}

        def wrap(ptr, n, typestr, dtype):
            if n == 0 or not ptr:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_Alias(ptr, n, typestr), device=dev)

        n, n_ops, n_sig, n_seq = int(res.n_reads), int(res.n_ops), int(res.n_samples), int(res.n_seq)
        batch = Batch(n_reads=n, sig=wrap(res.sig, n_sig + 8, "<i2", torch.int16), sig_off=wrap(res.sig_off, n + 1, "<i8", torch.int64),
                      digitisation=wrap(res.digitisation, n, "<f8", torch.float64), offset=wrap(res.offset, n, "<f8", torch.float64), range=wrap(res.range, n, "<f8", torch.float64),
                      query_start=wrap(res.query_start, n, "<i4", torch.int32), target_start=wrap(res.target_start, n, "<i4", torch.int32),
                      target_end=wrap(res.target_end, n, "<i4", torch.int32), seq=wrap(res.seq, n_seq, "|u1", torch.uint8), seq_off=wrap(res.seq_off, n + 1, "<i8", torch.int64),
                      op_n=wrap(res.op_n, n_ops, "<i4", torch.int32), op_t=wrap(res.op_t, n_ops, "|u1", torch.uint8), op_off=wrap(res.op_off, n + 1, "<i8", torch.int64),
                      on_device=True, n_ops=n_ops, all_matches=True)
        status = np.ctypeslib.as_array(C.cast(res.status_host, C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
        self._keep = keep
        return SimReads(batch=batch, status=status, status_device=wrap(res.status, n, "<i4", torch.int32), n_ops=n_ops, n_samples=n_sig, n_refused=int(res.n_refused))

    def kernel_ms(self):
        """HIP-event time of k_sim_ops and of k_sim_emit since the last call."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.pg_sim_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_sim_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def simulate_reads(levels, stdvs, dwells, k: int, seqs, first_read: int = 0, **kw):
    """One-shot SignalSimulator.generate: the arrays on the host (SimReads.to_host) plus n_ops, n_samples and n_refused."""
    with SignalSimulator(levels, stdvs, dwells, k, **kw) as sim:
        r = sim.generate(seqs, first_read=first_read)
        out = r.to_host()
        out.update(n_ops=r.n_ops, n_samples=r.n_samples, n_refused=r.n_refused)
        return out


def sim_walk(levels, stdvs, dwells, k: int, seq, read: int = 0, sig_move_offset: int = 0, rna: bool = False, seed: int = 0, digitisation: int = 8192, range_e4: int = 14676100,
             offset: int = 10, off_spread: int = 0, spread_pct: int = 50, lead: int = 0, lead_level: int = 0, lead_stdv: int = 0):
    """The rule for one read on the host (pg_sim_walk; no GPU needed): (status, ops uint32, samples int16, off_r)."""
    lib = _abi.load()
    p = _sim_params(k, sig_move_offset, rna, seed, digitisation, range_e4, offset, off_spread, spread_pct, lead, lead_level, lead_stdv)
    lv, sd, dw = (np.ascontiguousarray(a, dtype=np.uint32) for a in (levels, stdvs, dwells))
    s = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)
    ops = np.zeros(max(s.size, 1), np.uint32)
    n, st, off = C.c_uint64(), C.c_uint32(), C.c_int32()
    sig = np.zeros(0, np.int16)
    for _ in range(2):  # the first call counts the samples
        rc = lib.pg_sim_walk(C.byref(p), lv.ctypes.data, sd.ctypes.data, dw.ctypes.data, s.ctypes.data, s.size, read, ops.ctypes.data, sig.ctypes.data, sig.size, C.byref(n),
                             C.byref(st), C.byref(off))
        if rc != 0:
            raise PgError(rc, "pg_sim_walk: bad argument")
        if sig.size >= n.value:
            break
        sig = np.zeros(n.value, np.int16)
    ok = st.value == 0
    return int(st.value), ops[:s.size if ok else 0].copy(), sig[:n.value].copy(), int(off.value)
