"""Host-side mirror of the reference's MATLAB interface for the hot path.

    [file, signal, acq, track, solu, cmn] = initParameters()      initParameters.m:1-85
    Acquired = acquisition(file, signal, acq)                      acquisition.m:1
    [TckResultCT, CN0_Eph, countinx] = trackingCT(file, signal, track, Acquired)
                                                                   trackingCT.m:1
    [TckResultCT_pos, CN0_CT] = trackingCT_POS(file, signal, track, Acquired, countinx)
                                   tracking loop of trackingCT_POS_updated.m:1-413
    [TckResultCT_pos, navSolutionsCT] = trackingCT_POS_updated(file, signal, track, cmn, Acquired,
                                   TckResult_Eph, cnslxyz, eph, sbf, solu, countinx=countinx)
                                   the whole of trackingCT_POS_updated.m, positioning included
    [ephemeris, ALLTckResult, for_prest] = naviDecode_updated(Acquired, ALLTckResult)
                                                                   naviDecode_updated.m:1

Same names, same struct fields, same argument meaning; the work happens in the
HIP C-ABI library (abi.py). Differences forced by the language are documented
per function. Errors follow the reference: nothing acquired -> empty Acquired
(acquisition.m:84-85); "Not enough raw data" -> TckResultCT = [] (returned as
an empty StructArray); conditions where MATLAB raises -> GnssError.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import abi, synth


# ---------------------------------------------------------------------------
# initParameters.m
# ---------------------------------------------------------------------------
def initParameters(fileRoute: str | None = None):
    """Struct surface of initParameters.m:1-85 (Opensky defaults).

    file.fid (a MATLAB file handle opened at :35) has no Python equivalent: the
    core does positioned reads of file.fileRoute, or uses file.data (an int8
    numpy record held in host memory) / file.dev (a DeviceRecord in HBM).
    """
    file = SimpleNamespace(fileName="Opensky", fileRoute=fileRoute, skip=5000, skiptimeVT=100,
                           dataType=2, dataPrecision=1, data=None, dev=None)
    signal = SimpleNamespace(IF=4.58e6, Fs=58e6, Fc=1575.42e6, codeFreqBasis=1.023e6, ms=1e-3)
    signal.Sample = math.ceil(signal.Fs * signal.ms)
    signal.codelength = signal.codeFreqBasis * signal.ms
    acq = SimpleNamespace(prnList=list(range(1, 33)), freqStep=500, freqMin=-10000, datalen=20, L=10)
    acq.freqNum = int(2 * abs(acq.freqMin) / acq.freqStep + 1)
    track = SimpleNamespace(CorrelatorSpacing=0.5, DLLBW=2, DLLDamp=0.707, DLLGain=0.1, PLLBW=15,
                            PLLDamp=0.707, PLLGain=0.25, msToProcessCT_1ms=1000,
                            msToProcessCT_10ms=40000, ctPOS=3000, msToProcessVT=5000, pdi=1)
    solu = SimpleNamespace(iniPos=[22.328444770087565 / 180 * math.pi,
                                   114.1713630049711 / 180 * math.pi, 4],
                           navSolPeriod=20, mode=2)
    cmn = SimpleNamespace(doy=171, vtEnable=1, mltCorrON=[1, 0], cSpeed=299792458, equip="stereo")
    return file, signal, acq, track, solu, cmn


# ---------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------
class Context:
    """One gnss_ctx on one HIP device (stream, rocFFT plans, device buffers), or with
    `devices` a multi-device context (gnss_ctx_create_multi): acquisition and trackingCT deal
    their PRNs / channels round-robin over one member context per entry (a device may repeat)
    and merge the rows, bit-identical to one context; device-resident records and outputs
    belong to devices[0]."""

    def __init__(self, device: int = 0, devices=None):
        self.lib = abi.load()
        h = C.c_void_p()
        if devices is not None:
            devs = [int(d) for d in devices]
            arr = (C.c_int * len(devs))(*devs)
            st = self.lib.gnss_ctx_create_multi(arr, len(devs), C.byref(h))
            if st != abi.OK:
                raise abi.GnssError(st, f"gnss_ctx_create_multi(devices={devs}) failed")
            device = devs[0]
        else:
            st = self.lib.gnss_ctx_create(int(device), C.byref(h))
            if st != abi.OK:
                raise abi.GnssError(st, f"gnss_ctx_create(device={device}) failed")
        self.h = h
        self.device = device
        self.devices = list(devices) if devices is not None else [device]

    @property
    def members(self) -> int:
        return int(self.lib.gnss_ctx_members(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gnss_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st != abi.OK:
            raise abi.GnssError(st, (self.lib.gnss_last_error(self.h) or b"").decode())
        return st

    def timing(self) -> dict:
        t = abi.GnssTiming()
        self.check(self.lib.gnss_last_timing(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.GnssTiming._fields_}

    def set_profiling(self, on: bool):
        self.check(self.lib.gnss_ctx_set_profiling(self.h, 1 if on else 0))

    def set_window(self, nbytes: int):
        """Streaming: at most nbytes of IF resident in HBM per trackingCT call (0: the whole
        read range), gnss_ctx_set_window."""
        self.check(self.lib.gnss_ctx_set_window(self.h, int(nbytes)))

    def set_option(self, key: int, value: int):
        """Test hook: force one engine path (abi.OPT_*, gnss_ctx_set_option)."""
        self.check(self.lib.gnss_ctx_set_option(self.h, int(key), int(value)))

    def lane_path(self) -> int:
        """1 when the last trackingCT / correlate_step took its tap prefixes from the capture
        register for every lane span it used, 0 through the LDS slots (gnss_ctx_lane_path)."""
        return int(self.lib.gnss_ctx_lane_path(self.h))

    def drop_record(self, dev=None):
        """Multi-device contexts: drop the members' resident copies of a device record (a
        DeviceRecord, a device pointer, or None for all), gnss_ctx_drop_record; needed only when
        the record's bytes were rewritten outside the library."""
        if dev is None:
            ptr = None
        else:
            v = getattr(dev, "ptr", dev)
            ptr = v.value if isinstance(v, C.c_void_p) else int(v)
        self.check(self.lib.gnss_ctx_drop_record(self.h, C.c_void_p(ptr)))

    @property
    def resident_records(self) -> int:
        """Resident record copies held by the members (gnss_ctx_resident_records)."""
        return int(self.lib.gnss_ctx_resident_records(self.h))

    def set_acq_precision(self, fp64: bool):
        """Acquisition correlation at fp64 (the reference's precision, default) or the fp32
        fast mode (gnss_ctx_set_acq_precision)."""
        self.check(self.lib.gnss_ctx_set_acq_precision(self.h, 1 if fp64 else 0))


class DeviceRecord:
    """An IF record resident in this context's HBM (bytes = file bytes)."""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx.check(ctx.lib.gnss_dev_alloc(ctx.h, C.c_uint64(self.nbytes), C.byref(p)))
        self.ptr = p

    @classmethod
    def from_host(cls, ctx: Context, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.int8)
        r = cls(ctx, data.nbytes)
        ctx.check(ctx.lib.gnss_dev_upload(ctx.h, r.ptr, data.ctypes.data_as(C.c_void_p),
                                          C.c_uint64(data.nbytes)))
        return r

    def upload(self, data: np.ndarray, offset: int = 0):
        """Host bytes into the record at `offset` (gnss_dev_upload; a multi-device context's
        members drop their resident copies of the record)."""
        data = np.ascontiguousarray(data, dtype=np.int8)
        dst = C.c_void_p(self.ptr.value + int(offset))
        self.ctx.check(self.ctx.lib.gnss_dev_upload(self.ctx.h, dst, data.ctypes.data_as(C.c_void_p),
                                                    C.c_uint64(data.nbytes)))

    def download(self, offset: int = 0, nbytes: int | None = None) -> np.ndarray:
        n = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.empty(n, dtype=np.int8)
        src = C.c_void_p(self.ptr.value + int(offset))
        self.ctx.check(self.ctx.lib.gnss_dev_download(self.ctx.h, out.ctypes.data_as(C.c_void_p),
                                                      src, C.c_uint64(n)))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.gnss_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---------------------------------------------------------------------------
# struct marshalling
# ---------------------------------------------------------------------------
def to_c_file(file):
    f = abi.GnssFile()
    keep = []
    path = getattr(file, "fileRoute", None)
    data = getattr(file, "data", None)
    dev = getattr(file, "dev", None)
    if dev is not None:
        f.dev_data = dev.ptr
        f.nbytes = dev.nbytes
    elif data is not None:
        # the record's byte image (an int16 array is passed through as its bytes)
        arr = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.asarray(data, np.int8)
        arr = arr.reshape(-1).view(np.int8)
        keep.append(arr)
        f.data = arr.ctypes.data
        f.nbytes = arr.nbytes
    elif path:
        f.path = str(path).encode()
    else:
        raise abi.GnssError(abi.EARG, "file has no fileRoute, data or dev record")
    f.skip = int(file.skip)
    f.dataType = int(file.dataType)
    f.dataPrecision = int(file.dataPrecision)
    return f, keep


def to_c_signal(signal):
    s = abi.GnssSignal()
    s.IF, s.Fs, s.codeFreqBasis, s.ms = signal.IF, signal.Fs, signal.codeFreqBasis, signal.ms
    s.Sample = int(signal.Sample)
    s.codelength = signal.codelength
    return s


def to_c_acq(acq, prn_list=None):
    a = abi.GnssAcq()
    a.freqNum, a.freqMin, a.freqStep = int(acq.freqNum), float(acq.freqMin), float(acq.freqStep)
    a.datalen, a.L = int(acq.datalen), int(acq.L)
    keep = []
    if prn_list is not None:
        arr = np.ascontiguousarray(prn_list, dtype=np.int32)
        keep.append(arr)
        a.n_prn = len(arr)
        a.prn_list = arr.ctypes.data_as(C.POINTER(C.c_int32))
    return a, keep


def to_c_acquired(Acquired):
    a = abi.GnssAcquired()
    n = len(Acquired.sv)
    a.n = n
    for i in range(n):
        a.sv[i] = int(Acquired.sv[i])
        a.SNR[i] = float(Acquired.SNR[i])
        a.Doppler[i] = float(Acquired.Doppler[i])
        a.codedelay[i] = int(Acquired.codedelay[i])
        a.fineFreq[i] = float(Acquired.fineFreq[i])
    return a


def from_c_acquired(a) -> SimpleNamespace:
    n = a.n
    return SimpleNamespace(sv=np.array(a.sv[:n], dtype=np.int64),
                           SNR=np.array(a.SNR[:n]), Doppler=np.array(a.Doppler[:n]),
                           codedelay=np.array(a.codedelay[:n], dtype=np.int64),
                           fineFreq=np.array(a.fineFreq[:n]))


def to_c_track(track, taps=None, channels=None):
    t = abi.GnssTrack()
    for f in ["CorrelatorSpacing", "DLLBW", "DLLDamp", "DLLGain", "PLLBW", "PLLDamp", "PLLGain"]:
        setattr(t, f, float(getattr(track, f)))
    t.msToProcessCT_1ms = int(track.msToProcessCT_1ms)
    t.msToProcessCT_10ms = int(track.msToProcessCT_10ms)
    keep = []
    if taps is not None:
        arr = np.ascontiguousarray(taps, dtype=np.float64)
        keep.append(arr)
        t.n_taps = len(arr)
        t.tap_offsets = arr.ctypes.data_as(C.POINTER(C.c_double))
    if channels is not None:
        arr = np.ascontiguousarray(channels, dtype=np.int32)
        keep.append(arr)
        t.n_chan = len(arr)
        t.chan = arr.ctypes.data_as(C.POINTER(C.c_int32))
    return t, keep


class TrackOutBuffers:
    """Caller-allocated trackingCT outputs (see gnss_track_out in the header)."""

    def __init__(self, nsv: int, track, ntaps: int = 0, ctPOS: int | None = None):
        self.max_len = int(track.msToProcessCT_1ms) + 19 + int(track.msToProcessCT_10ms)
        if ctPOS is not None:  # trackingCT_POS_updated: one row per step
            self.max_len = int(ctPOS)
        self.rec = np.zeros((nsv, abi.NFIELDS, self.max_len))
        self.taps = np.zeros((nsv, 2, ntaps, self.max_len)) if ntaps else None
        self.len = np.zeros(nsv, dtype=np.int64)
        self.countinx = np.zeros(nsv, dtype=np.int32)
        self.cn0_cap = max(int(track.msToProcessCT_1ms) + 19, int(track.msToProcessCT_10ms) // 10) // 20 + 1
        if ctPOS is not None:
            self.cn0_cap = int(ctPOS) // 20 + 1
        self.CN0 = np.zeros((self.cn0_cap, nsv))
        o = abi.GnssTrackOut()
        o.max_len = self.max_len
        o.rec = self.rec.ctypes.data_as(C.POINTER(C.c_double))
        o.taps = self.taps.ctypes.data_as(C.POINTER(C.c_double)) if ntaps else None
        o.len = self.len.ctypes.data_as(C.POINTER(C.c_int64))
        o.countinx = self.countinx.ctypes.data_as(C.POINTER(C.c_int32))
        o.CN0_Eph = self.CN0.ctypes.data_as(C.POINTER(C.c_double))
        o.cn0_cap = self.cn0_cap
        self.c = o
        self.shape = (nsv, self.max_len, ntaps, self.cn0_cap)

    def fits(self, nsv: int, track, ntaps: int) -> bool:
        max_len = int(track.msToProcessCT_1ms) + 19 + int(track.msToProcessCT_10ms)
        cn0_cap = max(int(track.msToProcessCT_1ms) + 19, int(track.msToProcessCT_10ms) // 10) // 20 + 1
        return self.shape == (nsv, max_len, ntaps, cn0_cap)


class DeviceTrackOutBuffers(TrackOutBuffers):
    """TrackOutBuffers whose rec / taps live in HBM (gnss_track_out.flags = GNSS_OUT_DEVICE):
    torch float64 tensors on `device`, filled by the library's expansion kernel; len,
    countinx and CN0 stay host arrays. The multi-GPU path all-gathers these rows over
    RCCL without a host round trip (dist.gather_tracking_rows_device)."""

    def __init__(self, nsv: int, track, ntaps: int = 0, device="cuda:0", ctPOS: int | None = None):
        torch = abi.require_torch()
        super().__init__(nsv, track, 0, ctPOS)
        self.device = torch.device(device)
        self.rec = torch.zeros((nsv, abi.NFIELDS, self.max_len), dtype=torch.float64, device=self.device)
        self.taps = (torch.zeros((nsv, 2, ntaps, self.max_len), dtype=torch.float64, device=self.device)
                     if ntaps else None)
        self.c.rec = C.cast(C.c_void_p(self.rec.data_ptr()), C.POINTER(C.c_double))
        self.c.taps = C.cast(C.c_void_p(self.taps.data_ptr()), C.POINTER(C.c_double)) if ntaps else None
        self.c.flags = abi.OUT_DEVICE
        self.shape = (nsv, self.max_len, ntaps, self.cn0_cap)

    def sync_producer(self):
        """The library writes on its own stream: torch's pending work on these tensors
        (allocation fill, an all-gather) must be done first."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    def host(self) -> TrackOutBuffers:
        """A host copy (TrackOutBuffers) of the same result."""
        h = TrackOutBuffers.__new__(TrackOutBuffers)
        h.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("device",)})
        h.rec = self.rec.cpu().numpy()
        h.taps = self.taps.cpu().numpy() if self.taps is not None else None
        return h


class StructArray:
    """MATLAB struct array indexed by PRN: TckResultCT(prn).P_i (trackingCT.m:153)."""

    def __init__(self, entries: dict):
        self._e = entries

    def __call__(self, prn):
        return self._e[int(prn)]

    def __len__(self):
        return max(self._e) if self._e else 0

    def __bool__(self):
        return bool(self._e)

    def prns(self):
        return sorted(self._e)


def build_tck_result(Acquired, buf: TrackOutBuffers, channels=None, fields=None) -> StructArray:
    entries = {}
    chans = range(len(Acquired.sv)) if channels is None else channels
    fields = fields or abi.FIELDS
    for c in chans:
        n = int(buf.len[c])
        e = SimpleNamespace(**{f: buf.rec[c, k, :n].copy() for k, f in enumerate(fields)})
        if buf.taps is not None:
            e.taps_i = buf.taps[c, 0, :, :n].copy()
            e.taps_q = buf.taps[c, 1, :, :n].copy()
        entries[int(Acquired.sv[c])] = e
    return StructArray(entries)


# ---------------------------------------------------------------------------
# acquisition.m / trackingCT.m
# ---------------------------------------------------------------------------
def acquisition(file, signal, acq, *, ctx: Context | None = None, prn_list=None,
                diag: bool = False):
    """acquisition.m:1-127 on the GPU.

    Like the reference, acq.prnList is ignored (acquisition.m:47 hard-codes 1:32,
    quirk A.1); `prn_list` selects PRNs explicitly (config 1: [3]; rank sharding).
    Returns Acquired (fields sv, SNR, Doppler, codedelay, fineFreq as row vectors),
    plus the per-PRN detector diagnostics when diag=True.
    """
    ctx = ctx or default_context()
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    a, k2 = to_c_acq(acq, prn_list)
    out = abi.GnssAcquired()
    dg = abi.GnssAcqDiag()
    st = ctx.lib.gnss_acquisition(ctx.h, C.byref(f), C.byref(s), C.byref(a), C.byref(out),
                                  C.byref(dg))
    if st not in (abi.OK, abi.ENODATA):
        ctx.check(st)
    if st == abi.ENODATA:
        print("No satellites acquired. Check parameter settings ... \n")
    res = from_c_acquired(out)
    if diag:
        n = dg.n
        d = SimpleNamespace(prn=np.array(dg.prn[:n]), SNR=np.array(dg.SNR[:n]),
                            fbin=np.array(dg.fbin[:n]), codePhase=np.array(dg.codePhase[:n]),
                            peak=np.array(dg.peak[:n]), peak2=np.array(dg.peak2[:n]))
        return res, d
    return res


def acquisition_surface(file, signal, acq, *, ctx: Context | None = None, prn_list=None):
    """The acquisition's whole correlation surface (gnss_acquisition_surface, a parity hook):
    the coarse half of `acquisition` under the context's precision and options, no fine search.
    Returns (surface[np, freqNum, Sample] in natural column order, as float64; the per-PRN
    detector diagnostics the same call computed from it)."""
    ctx = ctx or default_context()
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    a, k2 = to_c_acq(acq, prn_list)
    npr = len(prn_list) if prn_list is not None else 32
    surf = np.zeros((npr, int(acq.freqNum), int(signal.Sample)))
    dg = abi.GnssAcqDiag()
    st = ctx.lib.gnss_acquisition_surface(ctx.h, C.byref(f), C.byref(s), C.byref(a),
                                          surf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(dg))
    ctx.check(st)
    n = dg.n
    d = SimpleNamespace(prn=np.array(dg.prn[:n]), SNR=np.array(dg.SNR[:n]),
                        fbin=np.array(dg.fbin[:n]), codePhase=np.array(dg.codePhase[:n]),
                        peak=np.array(dg.peak[:n]), peak2=np.array(dg.peak2[:n]))
    return surf, d


def trackingCT(file, signal, track, Acquired, *, ctx: Context | None = None, taps=None,
               channels=None, save_countinx: str | None = None, raw: bool = False,
               out: "TrackOutBuffers | None" = None):
    """trackingCT.m:1-530 on the GPU -> (TckResultCT, CN0_Eph, countinx).

    TckResultCT is indexed by PRN (TckResultCT(prn).P_i), CN0_Eph is
    cn0_rows x nsv, countinx is 1 x nsv. `taps` enables the multi-correlator ACF
    taps (config 5); `channels` tracks a subset (multi-GPU shard). The side file
    countinx.mat of trackingCT.m:530 is written only when save_countinx names it.
    With raw=True the TrackOutBuffers are returned instead of the structs; `out` reuses
    a TrackOutBuffers of the same shape from an earlier call (no 10s of MB allocated and
    freed per call; rows of channels outside `channels` keep their old contents).
    """
    ctx = ctx or default_context()
    nsv = len(Acquired.sv)
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    t, k2 = to_c_track(track, taps, channels)
    a = to_c_acquired(Acquired)
    ntaps = 0 if taps is None else len(taps)
    if out is not None and out.fits(nsv, track, ntaps):
        buf = out
        buf.len[:] = 0
        buf.countinx[:] = 0
    else:
        buf = TrackOutBuffers(nsv, track, ntaps)
    if isinstance(buf, DeviceTrackOutBuffers):
        buf.sync_producer()
    st = ctx.lib.gnss_tracking_ct(ctx.h, C.byref(f), C.byref(s), C.byref(t), C.byref(a),
                                  C.byref(buf.c))
    if st == abi.ENODATA:
        print("Not enough raw data  \n")
        return StructArray({}), np.zeros((0, nsv)), buf.countinx.astype(np.int64)
    ctx.check(st)
    if raw:
        return buf
    countinx = buf.countinx.astype(np.int64)
    if save_countinx:
        import scipy.io as sio
        sio.savemat(save_countinx, {"countinx": countinx.reshape(1, -1)})
    cn0 = buf.CN0[: buf.c.cn0_rows].copy()
    hb = buf.host() if isinstance(buf, DeviceTrackOutBuffers) else buf
    return build_tck_result(Acquired, hb, channels), cn0, countinx


def trackingCT_POS(file, signal, track, Acquired, countinx, *, ctx: Context | None = None,
                   channels=None, raw: bool = False):
    """The tracking loop of trackingCT_POS_updated.m (:92-144, :179-413) on the GPU ->
    (TckResultCT_pos, CN0_CT).

    The reference reads `countinx` from countinx.mat (:29) and indexes it by the channel's
    position in Acquired (quirk A.17); pass that vector here. track.ctPOS is the step count
    (datalength, :50). The positioning half of the reference function (pseudoranges,
    least squares, :420-565) is ct_positioning / trackingCT_POS_updated: TckResultCT_pos carries the fields of
    :273-292 (E_i ... delayValue, absoluteSampleCodedelay) per PRN, one row per step.
    """
    ctx = ctx or default_context()
    nsv = len(Acquired.sv)
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    t, k2 = to_c_track(track, None, channels)
    a = to_c_acquired(Acquired)
    cx = np.ascontiguousarray(np.asarray(countinx).reshape(-1)[:nsv], dtype=np.int32)
    ctPOS = int(track.ctPOS)
    buf = TrackOutBuffers(nsv, track, 0, ctPOS=ctPOS)
    st = ctx.lib.gnss_tracking_ct_pos(ctx.h, C.byref(f), C.byref(s), C.byref(t), C.byref(a),
                                      ctPOS, cx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(buf.c))
    ctx.check(st)
    if raw:
        return buf
    cn0 = buf.CN0[: buf.c.cn0_rows].copy()
    return build_tck_result(Acquired, buf, channels, abi.FIELDS_POS), cn0


def mc_result(Acquired, buf: TrackOutBuffers, channels=None, fields=None) -> StructArray:
    """TckResultCT_mltCorr: the loop fields plus every tap under the reference's names
    (E_i_060 ... P_i ... L_q060, trackingCT_POS_updated_multicorrelator.m:374-439,
    trackingCT_multiCorr-GIVEN.m:248-286)."""
    res = build_tck_result(Acquired, buf, channels, fields or abi.FIELDS_POS)
    for prn in res.prns():
        e = res(prn)
        for k, name in enumerate(abi.MC_TAP_NAMES):
            setattr(e, name.format("i"), e.taps_i[k])
            setattr(e, name.format("q"), e.taps_q[k])
    return res


def trackingCT_POS_updated_multicorrelator(file, signal, track, Acquired, *,
                                           ctx: Context | None = None, channels=None,
                                           raw: bool = False, device_records: bool = False):
    """The tracking loop of trackingCT_POS_updated_multicorrelator.m (:41-136, :170-440) on
    the GPU -> (TckResultCT_mltCorr, CN0_CT).

    track.msPosCT (datalength, :49; initParameters.m does not define it, the caller sets
    it) and track.pdi (:46, 1 or 10) give msPosCT/pdi steps, every one at that pdi. The 25
    taps at Spacing = 0.6:-0.05:-0.6 are all recorded; E/P/L = Spacing(3)/(13)/(23) drive
    the loops. The positioning half (:446-590) is ct_positioning(..., mode="multicorr") on
    the returned records. With device_records the records and taps stay in HBM
    (DeviceTrackOutBuffers, GNSS_OUT_DEVICE): with raw they are returned as they lie, for
    acf_features / ct_positioning to read there.
    """
    ctx = ctx or default_context()
    nsv = len(Acquired.sv)
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    t, k2 = to_c_track(track, None, channels)
    a = to_c_acquired(Acquired)
    msPosCT, pdi = int(track.msPosCT), int(track.pdi)
    nsteps = msPosCT // pdi if pdi > 0 else 0
    if device_records:
        buf = DeviceTrackOutBuffers(nsv, track, abi.MC_TAPS, device=f"cuda:{ctx.device}", ctPOS=max(nsteps, 1))
        buf.sync_producer()
    else:
        buf = TrackOutBuffers(nsv, track, abi.MC_TAPS, ctPOS=max(nsteps, 1))
    st = ctx.lib.gnss_tracking_ct_mc(ctx.h, C.byref(f), C.byref(s), C.byref(t), C.byref(a),
                                     msPosCT, pdi, C.byref(buf.c))
    ctx.check(st)
    buf.acf_orient = abi.ACF_ORIENT["trackingCT_POS_updated_multicorrelator"]  # (acf_fit reads it)
    if raw:
        return buf
    if device_records:
        buf = buf.host()
    cn0 = buf.CN0[: buf.c.cn0_rows].copy()
    res = mc_result(Acquired, buf, channels)
    res.acf_orient = buf.acf_orient
    return res, cn0


def trackingCT_multiCorr(file, signal, track, Acquired, *, datalength: int = 50000,
                         ctx: Context | None = None, raw: bool = False):
    """trackingCT_multiCorr-GIVEN.m (function trackingCT_multiCorr) on the GPU ->
    (TckResultCT, CN0_CT).

    `datalength` 1-ms steps per channel (:27 hard-codes 50000) from fseek(Sample - codedelay
    - 1 + skip*Sample) (:57), trackingCT.m's loop with ceil numSample on the 25 taps
    Spacing = -0.6:0.05:0.6. TckResultCT(prn) carries the trackingCT field names of :287-297
    plus E_i_060 ... L_q060; codedelay keeps the reference's linear sum over one shared
    nsv x datalength delayValue matrix (earlier channels' rows included).
    """
    ctx = ctx or default_context()
    nsv = len(Acquired.sv)
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    t, k2 = to_c_track(track, None, None)
    a = to_c_acquired(Acquired)
    buf = TrackOutBuffers(nsv, track, abi.MC_TAPS, ctPOS=max(int(datalength), 1))
    st = ctx.lib.gnss_tracking_ct_multicorr(ctx.h, C.byref(f), C.byref(s), C.byref(t), C.byref(a),
                                            int(datalength), C.byref(buf.c))
    ctx.check(st)
    buf.acf_orient = abi.ACF_ORIENT["trackingCT_multiCorr"]  # (acf_fit reads it)
    if raw:
        return buf
    res = mc_result(Acquired, buf, None, abi.FIELDS)
    res.acf_orient = buf.acf_orient
    return res, buf.CN0[: buf.c.cn0_rows].copy()


def naviDecode_updated(Acquired, ALLTckResult, *, eph_cap: int = 512):
    """naviDecode_updated.m:1-253 -> (ephemeris, ALLTckResult, for_prest).

    ALLTckResult(prn).P_i is read for every PRN of Acquired.sv, in that order (the
    reference's channel order matters: its bit arrays carry over between channels).
    ephemeris(prn) has the ini_eph.m fields as row vectors plus updateflag; for_prest.nav1
    / for_prest.sfb1 are indexed by PRN like the MATLAB vectors (nav1 has max(sv) entries,
    sfb1 ends at the last PRN that decoded a subframe 1). ALLTckResult is returned as given
    with .sfb1 added per PRN (the reference's second output). Host code (csrc/navdecode.cpp).
    """
    lib = abi.load()
    sv = [int(x) for x in Acquired.sv]
    n = len(sv)
    series = [np.ascontiguousarray(ALLTckResult(p).P_i, dtype=np.float64).ravel() for p in sv]
    stride = max(len(x) for x in series)
    P = np.zeros((n, stride))
    for i, x in enumerate(series):
        P[i, : len(x)] = x
    lens = np.array([len(x) for x in series], dtype=np.int64)
    eph = np.zeros((n, abi.EPH_NFIELDS, eph_cap))
    elen = np.zeros((n, abi.EPH_NFIELDS), dtype=np.int32)
    upd = np.zeros(n, dtype=np.int32)
    nav1 = np.zeros(n, dtype=np.int64)
    sfb1 = np.zeros(n, dtype=np.int64)
    o = abi.GnssNavOut()
    o.eph_cap = eph_cap
    o.eph = eph.ctypes.data_as(C.POINTER(C.c_double))
    o.eph_len = elen.ctypes.data_as(C.POINTER(C.c_int32))
    o.updateflag = upd.ctypes.data_as(C.POINTER(C.c_int32))
    o.nav1 = nav1.ctypes.data_as(C.POINTER(C.c_int64))
    o.sfb1 = sfb1.ctypes.data_as(C.POINTER(C.c_int64))
    a = to_c_acquired(Acquired)
    st = lib.gnss_navi_decode(C.byref(a), P.ctypes.data_as(C.POINTER(C.c_double)),
                              lens.ctypes.data_as(C.POINTER(C.c_int64)), stride, C.byref(o))
    if st != abi.OK:
        raise abi.GnssError(st, "gnss_navi_decode")
    entries = {}
    for i, p in enumerate(sv):
        e = SimpleNamespace(**{f: eph[i, k, : elen[i, k]].copy() for k, f in enumerate(abi.EPH_FIELDS)})
        e.updateflag = int(upd[i])
        entries[p] = e
    n1 = np.zeros(max(sv), dtype=np.int64)
    for i, p in enumerate(sv):
        n1[p - 1] = nav1[i]
    have = [p for i, p in enumerate(sv) if sfb1[i]]
    s1 = np.zeros(max(have) if have else 0, dtype=np.int64)
    for i, p in enumerate(sv):
        if sfb1[i]:
            s1[p - 1] = sfb1[i]
    for i, p in enumerate(sv):
        try:
            ALLTckResult(p).sfb1 = entries[p].sfb1.copy()
        except (AttributeError, TypeError):
            pass
    return StructArray(entries), ALLTckResult, SimpleNamespace(nav1=n1, sfb1=s1)


def colon(a: float, d: float, b: float) -> np.ndarray:
    """MATLAB's a:d:b with MathWorks' published colon construction (both ends toward the
    midpoint), the values the reference's tap vectors hold (e.g. -0.5:0.1:0.5 of the
    11-tap ACF, trackingCT_multiCorr-GIVEN.m:25). Same arithmetic as colon_make in
    csrc/gnss_internal.h."""
    if d == 0 or (a < b and d < 0) or (b < a and d > 0):
        return np.zeros(0)
    tol = 2.0 * 2.220446049250313e-16 * max(abs(a), abs(b))
    sig = 1.0 if d > 0 else -1.0
    if a == math.floor(a) and d == 1:
        n = math.floor(b) - a
    elif a == math.floor(a) and d == math.floor(d):
        q = math.floor(a / d)
        n = math.floor((b - (a - q * d)) / d) - q
    else:
        n = round((b - a) / d)  # (b - a)/d is never a half-integer for these ranges
        if sig * (a + n * d - b) > tol:
            n -= 1
    n = int(n)
    c = a + n * d
    if sig * (c - b) > -tol:
        c = b
    out = np.empty(n + 1)
    for k in range(n + 1):
        out[k] = (a + c) / 2 if 2 * k == n else (a + k * d if k <= n // 2 else c - (n - k) * d)
    return out


def ca_code(prn: int) -> np.ndarray:
    """generateCAcode(PRN) as used by the kernels (1023 chips of +-1)."""
    lib = abi.load()
    out = np.zeros(1023, dtype=np.int8)
    st = lib.gnss_ca_code(int(prn), out.ctypes.data_as(C.c_void_p))
    if st != abi.OK:
        raise abi.GnssError(st, "gnss_ca_code")
    return out


def vt_channel(prn, file_ptr, remChip, remCarrPhase, codeFreq, carrFreq, carrFreqBasis, oldCarrNco=0.0,
               oldCarrError=0.0):
    """A vector-tracking channel state (gnss_vt_chan): the initialisation of
    trackingVT_POS_updated.m:108-125 (from TckResultCT at msStartTckVT in the reference) and
    of the C/N0 estimator (:78-81: index_int 0, snrIndex 1)."""
    return abi.GnssVtChan(prn=int(prn), pad=0, file_ptr=int(file_ptr), remChip=float(remChip),
                          remCarrPhase=float(remCarrPhase), codeFreq=float(codeFreq), carrFreq=float(carrFreq),
                          carrFreqBasis=float(carrFreqBasis), oldCarrNco=float(oldCarrNco),
                          oldCarrError=float(oldCarrError), index_int=0, snrIndex=1)


def trackingVT_step(file, signal, track, chans, codeFreq_new, pdi=1, *, ctx: Context | None = None):
    """One step of trackingVT_POS_updated.m's tracking half (:157-349) for every channel on the
    GPU (gnss_tracking_vt_step): `chans` = a sequence of vt_channel states, advanced in place;
    codeFreq_new[i] = channel i's code frequency for this step, the caller's EKF prediction
    (:211-215). Returns one dict per channel: TckResultVT(prn).*(msIndex) (:319-346)."""
    ctx = ctx or default_context()
    n = len(chans)
    arr = (abi.GnssVtChan * n)(*chans)
    cf = np.ascontiguousarray(codeFreq_new, dtype=np.float64)
    if len(cf) != n:
        raise ValueError("one code frequency per channel")
    outs = (abi.GnssVtOut * n)()
    f, keep = to_c_file(file)
    s = to_c_signal(signal)
    t, keep2 = to_c_track(track)
    ctx.check(ctx.lib.gnss_tracking_vt_step(ctx.h, C.byref(f), C.byref(s), C.byref(t), int(pdi), n, arr,
                                            cf.ctypes.data_as(C.POINTER(C.c_double)), outs))
    for i in range(n):
        C.memmove(C.byref(chans[i]), C.byref(arr[i]), C.sizeof(abi.GnssVtChan))
    return [{k: (getattr(o, k)[:] if k == "sv_vel" else getattr(o, k)) for k, _ in abi.GnssVtOut._fields_}
            for o in outs]


def trackingVT_run(file, signal, track, chans, codeFreq_series, pdi=1, *, ctx: Context | None = None):
    """nsteps steps of trackingVT_POS_updated.m's tracking half (:157-349) for every channel in
    ONE launch (gnss_tracking_vt_run): codeFreq_series[s][i] = channel i's code frequency of
    step s (the caller's EKF prediction, :211-215, or a recorded series); `chans` advanced in
    place. Returns a dict of [nsteps][n] arrays: TckResultVT(prn).*(msIndex) (:319-346), CN0
    and cn0_row (CN0_VT(cn0_row, svindex), :301), status."""
    ctx = ctx or default_context()
    n = len(chans)
    cf = np.ascontiguousarray(codeFreq_series, dtype=np.float64)
    if cf.ndim != 2 or cf.shape[1] != n:
        raise ValueError("codeFreq_series: [nsteps][n]")
    nsteps = cf.shape[0]
    arr = (abi.GnssVtChan * n)(*chans)
    outs = (abi.GnssVtOut * (nsteps * n))()
    f, keep = to_c_file(file)
    s = to_c_signal(signal)
    t, keep2 = to_c_track(track)
    st = ctx.lib.gnss_tracking_vt_run(ctx.h, C.byref(f), C.byref(s), C.byref(t), int(pdi), n, nsteps, arr,
                                      cf.ctypes.data_as(C.POINTER(C.c_double)), outs)
    for i in range(n):
        C.memmove(C.byref(chans[i]), C.byref(arr[i]), C.sizeof(abi.GnssVtChan))
    rec = np.ctypeslib.as_array(outs).reshape(nsteps, n)  # a structured view of the records
    ctx.check(st)
    return {k: rec[k].copy() for k in rec.dtype.names}


def correlate_step(file, signal, prn, pdi, remChip, codeFreq, carrierFreq, remPhase, pos_bytes,
                   taps, *, ctx: Context | None = None):
    """One trackingCT correlation step on the GPU at an arbitrary NCO state
    (trackingCT.m:79-118 without negation / loop update). Returns (sums, numSample)
    with sums = [I_0, Q_0, I_1, Q_1, ...] per tap."""
    ctx = ctx or default_context()
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    sums = np.zeros(2 * len(taps))
    ns = C.c_int64()
    ctx.check(ctx.lib.gnss_correlate_step(
        ctx.h, C.byref(f), C.byref(s), int(prn), int(pdi), float(remChip), float(codeFreq),
        float(carrierFreq), float(remPhase), int(pos_bytes), len(taps),
        taps.ctypes.data_as(C.POINTER(C.c_double)), sums.ctypes.data_as(C.POINTER(C.c_double)),
        C.byref(ns)))
    return sums, ns.value


# ---------------------------------------------------------------------------
# trackingVT_POS_updated.m: the EKF-driven vector-tracking loop
# ---------------------------------------------------------------------------
# global ALPHA BETA of initParameters.m:29-31 (the broadcast iono model, "From RINEX file")
ALPHA = [9.3132e-09, 1.4901e-08, -5.9605e-08, -1.1921e-07]
BETA = [8.8064e+04, 4.9152e+04, -1.3107e+05, -3.2768e+05]

VT_FIELDS = ["E_i", "E_q", "P_i", "P_q", "L_i", "L_q", "carrError", "codeError", "remChip", "remCarrPhase",
             "codeFreq", "carrFreq", "carrNco", "absoluteSample", "codedelay", "deltaPr", "prRate"]


def _struct_of(s, prn):
    """eph(prn) / TckResultCT(prn): a StructArray (or any callable), a dict keyed by PRN, or a
    sequence indexed like the MATLAB struct array (prn - 1)."""
    if callable(s):
        return s(prn)
    if isinstance(s, dict):
        return s[int(prn)]
    return s[int(prn) - 1]


def _first(x):
    return float(np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel()[0])


def _vec1(v, prn):
    """sbf.nav1(prn): MATLAB 1-based vector indexing."""
    return _first(np.asarray(v).ravel()[int(prn) - 1])


def eph_sv(eph, prn, eph_idx=1):
    """The gnss_eph_sv of ephemeris(prn).*(eph_idx) (svPosVel.m:23-44; the VT loop passes
    eph_idx = 1, trackingVT_POS_updated.m:36)."""
    e = _struct_of(eph, prn)
    out = abi.GnssEphSv()
    for f in abi.EPH_SV_FIELDS:
        setattr(out, f, float(np.atleast_1d(np.asarray(getattr(e, f), dtype=np.float64)).ravel()[eph_idx - 1]))
    return out


def trackingVT_POS_updated(file, signal, track, cmn, solu, Acquired, cnslxyz, eph, sbf, TckResult_Eph,
                           TckResultCT, navSolutionsCT, *, ctx: Context | None = None, ALPHA_=None,
                           BETA_=None, nsteps: int | None = None, return_cn0: bool = False):
    """trackingVT_POS_updated.m:1-476 -> (TckResultVT, navSolutionsVT[, CN0_VT]).

    The loop of track.msToProcessVT / track.pdi steps: per step and channel the read size (:164)
    and the code frequency predicted from the EKF's receiver state (:180-227; host,
    gnss_vt_nav_predict), the E/P/L correlations, NCO, PLL and C/N0 of every channel in one
    GPU launch (:229-352), then the 8-state EKF on the code and carrier measurements
    (:357-467; host, gnss_vt_nav_update) -- all inside gnss_tracking_vt.

    Initialisation as the reference: the EKF state from navSolutionsCT row
    file.skiptimeVT / solu.navSolPeriod (:66-70), the channels from TckResultCT(prn) at
    msStartTckVT (:100-124: built from the LAST channel's sbf.nav1 / eph.sfb(1) and capped at
    that channel's record length, as the reference's loop variable leaves them),
    transmitTimeVT = navSolutionsCT.timeTransmit(1, :) (:131). TckResult_Eph only feeds
    sampleStart (:89-99), which no output reads; it is index-checked like MATLAB when given
    (the reference ships none: None skips the check). ALPHA_ / BETA_ default to
    initParameters.m's globals. nsteps overrides datalength / pdi (a shorter run).

    TckResultVT(prn) carries the fields of :324-352 (sv_vel as nsteps x 3; amplitude,
    navi_data, navi_dataL035 are the constant 0 the reference records); navSolutionsVT the
    rows of :418-436 (svxyz_pos n x 3 x nsteps, kalman_gain 8 x 2n x nsteps as the
    reference's 3-D arrays) and R (:466). A channel error MATLAB raises on (a replica index
    out of range, a read past the end of the record) raises GnssError.
    """
    R, sols, sv, nsteps = _vt_loop(file, signal, track, cmn, solu, Acquired, cnslxyz, eph, sbf, TckResult_Eph,
                                   TckResultCT, navSolutionsCT, ctx, ALPHA_, BETA_, nsteps, True,
                                   "gnss_tracking_vt", abi.GnssVtOut)
    n = len(sv)
    entries = {}
    for i, p in enumerate(sv):
        e = SimpleNamespace(**{k: R[k][:, i].astype(np.float64) for k in VT_FIELDS})
        e.sv_vel = R["sv_vel"][:, i].copy()
        for k in ("amplitude", "navi_data", "navi_dataL035"):
            setattr(e, k, np.zeros(nsteps))
        entries[p] = e
    nsol = _navsol_arrays(sols, nsteps, n)
    TckResultVT = StructArray(entries)
    if return_cn0:
        return TckResultVT, nsol, _cn0_rows(R, nsteps, n)
    return TckResultVT, nsol


def _cn0_rows(R, nsteps, n):
    """CN0_VT (rows x channels) from the records' cn0_row / CN0."""
    rows = int(R["cn0_row"].max()) if nsteps else 0
    cn0 = np.zeros((rows, n))
    for i in range(n):
        m = R["cn0_row"][:, i] > 0
        cn0[R["cn0_row"][:, i][m] - 1, i] = R["CN0"][:, i][m]
    return cn0


def _vt_loop(file, signal, track, cmn, solu, Acquired, cnslxyz, eph, sbf, TckResult_Eph, TckResultCT,
             navSolutionsCT, ctx, ALPHA_, BETA_, nsteps, clamp, entry, OutT):
    """The initialisation both vector-tracking loops share (trackingVT_POS_updated.m:66-132; the
    25-tap loop's :63-123 is the same without the msStartTckVT clamp of the plain file's :106,
    `clamp`), then the library's loop `entry` -> (records [nsteps][n] as a structured array of
    OutT, the gnss_vt_navsol rows, the PRNs, nsteps)."""
    ctx = ctx or default_context()
    sv = [int(p) for p in np.atleast_1d(Acquired.sv)]
    n = len(sv)
    if not 1 <= n <= abi.VT_MAX_CH:
        raise ValueError(f"vector tracking takes 1..{abi.VT_MAX_CH} channels")
    pdi = int(track.pdi)
    if nsteps is None:
        nsteps = int(track.msToProcessVT) // pdi
    row = file.skiptimeVT / solu.navSolPeriod
    if row != int(row) or row < 1:
        raise IndexError("file.skiptimeVT / solu.navSolPeriod must be a positive integer row (:66)")
    row = int(row)
    # :89-107
    if TckResult_Eph is not None:
        for p in sv:
            k = int(_vec1(sbf.nav1, p) + _first(_struct_of(eph, p).sfb) * 20)
            np.asarray(_struct_of(TckResult_Eph, p).absoluteSample).ravel()[k - 1]  # MATLAB's index check
    last = sv[-1]
    ms = int(_vec1(sbf.nav1, last) + _first(_struct_of(eph, last).sfb) * 20 + row)
    if clamp:
        ms = min(ms, np.asarray(_struct_of(TckResultCT, last).codeFreq).size)
    chans = []
    for p in sv:  # :109-132
        t = _struct_of(TckResultCT, p)
        g = lambda f: float(np.asarray(getattr(t, f), dtype=np.float64).ravel()[ms - 1])
        c = vt_channel(p, int(g("absoluteSample")), g("remChip"), g("remCarrPhase"), g("codeFreq"),
                       g("carrFreq"), g("carrFreq"), g("carrFreq") - g("carrFreq"), g("carrError"))
        chans.append(c)
    arr = (abi.GnssVtChan * n)(*chans)
    cfg = abi.GnssVtNavCfg()
    cfg.cnslxyz[:] = [float(x) for x in np.asarray(cnslxyz, dtype=np.float64).ravel()[:3]]
    cfg.ALPHA[:] = [float(x) for x in (ALPHA_ if ALPHA_ is not None else ALPHA)]
    cfg.BETA[:] = [float(x) for x in (BETA_ if BETA_ is not None else BETA)]
    cfg.doy, cfg.cSpeed, cfg.Fc = float(cmn.doy), float(cmn.cSpeed), float(signal.Fc)
    ephs = (abi.GnssEphSv * n)(*[eph_sv(eph, p) for p in sv])
    ns = navSolutionsCT
    pos = (C.c_double * 3)(*np.asarray(ns.usrPos, dtype=np.float64)[row - 1, :3])
    vel = (C.c_double * 3)(*np.asarray(ns.usrVel, dtype=np.float64)[row - 1, :3])
    tt = (C.c_double * n)(*np.asarray(ns.timeTransmit, dtype=np.float64).reshape(-1, n)[0])
    s = to_c_signal(signal)
    nav = abi.GnssVtNav()
    st = ctx.lib.gnss_vt_nav_init(C.byref(cfg), C.byref(s), pdi, n, (C.c_int32 * n)(*sv), ephs, pos, vel,
                                  _vec1(ns.clkBias, row), _vec1(ns.clkDrift, row), tt, C.byref(nav))
    if st != abi.OK:
        raise abi.GnssError(st, "gnss_vt_nav_init")
    outs = (OutT * (nsteps * n))()
    sols = (abi.GnssVtNavSol * nsteps)()
    f, keep = to_c_file(file)
    t, keep2 = to_c_track(track)
    st = getattr(ctx.lib, entry)(ctx.h, C.byref(f), C.byref(s), C.byref(t), n, nsteps, arr, C.byref(nav), outs, sols)
    ctx.check(st)
    R = np.ctypeslib.as_array(outs).reshape(nsteps, n).copy()  # the records as a structured array
    return R, sols, sv, nsteps


def _navsol_arrays(sols, nsteps, n):
    """navSolutionsVT (:418-436, :466) from the gnss_vt_navsol rows."""
    N = 2 * n
    S = np.ctypeslib.as_array(sols).reshape(nsteps)
    out = SimpleNamespace(**{k: S[k].copy() for k in ("localTime", "clkBias", "clkDrift")})
    for k in ("usrPos", "usrVel", "usrPosENU", "usrVelENU", "usrPosLLH", "satePos", "sateVel", "state",
              "state_cov"):
        setattr(out, k, S[k].copy())
    for k in ("meas_inno", "newZ", "predicted_z"):
        setattr(out, k, S[k][:, :N].copy())
    for k in ("satEA", "satAZ"):
        setattr(out, k, S[k][:, :n].copy())
    out.svxyz_pos = np.moveaxis(S["svxyz_pos"][:, :n], 0, -1).copy()          # n x 3 x nsteps
    out.kalman_gain = np.moveaxis(S["kalman_gain"][:, :, :N], 0, -1).copy()   # 8 x 2n x nsteps
    out.R = S["R"][S["r_row"] > 0][:, :N].copy()
    out.record_correction = np.zeros((nsteps, n))  # correction(svindex) = 0 (:128, :469)
    return out


# ---------------------------------------------------------------------------
# trackingVT_POS_updated_multicorrelator.m: the 25-tap vector-tracking loop
# ---------------------------------------------------------------------------
def _mc_tap_fields(e, R, i):
    """The 50 sums of channel i under the reference's names (E_i_060 ... L_q060, :401-450)."""
    for k, name in enumerate(abi.MC_TAP_NAMES):
        setattr(e, name.format("i"), R["tap_i"][:, i, k].copy())
        setattr(e, name.format("q"), R["tap_q"][:, i, k].copy())


def trackingVT_mc_run(file, signal, track, chans, codeFreq_series, pdi=1, *, ctx: Context | None = None):
    """nsteps steps of trackingVT_POS_updated_multicorrelator.m's tracking half (:151-470) for
    every channel, one launch of the 25-tap correlator per step (gnss_tracking_vt_mc_run):
    codeFreq_series[s][i] = channel i's code frequency of step s (the caller's EKF prediction,
    :209-214); `chans` (vt_channel states) advanced in place. Returns a dict of [nsteps][n]
    arrays: the fields of trackingVT_run plus tap_i / tap_q [nsteps][n][25] in Spacing order
    (0.6:-0.05:-0.6; E / P / L = taps 2 / 12 / 22). The records are in `GnssError.records` when a
    channel stops (its status set)."""
    ctx = ctx or default_context()
    n = len(chans)
    cf = np.ascontiguousarray(codeFreq_series, dtype=np.float64)
    if cf.ndim != 2 or cf.shape[1] != n:
        raise ValueError("codeFreq_series: [nsteps][n]")
    nsteps = cf.shape[0]
    arr = (abi.GnssVtChan * n)(*chans)
    outs = (abi.GnssVtMcOut * (nsteps * n))()
    f, keep = to_c_file(file)
    s = to_c_signal(signal)
    t, keep2 = to_c_track(track)
    st = ctx.lib.gnss_tracking_vt_mc_run(ctx.h, C.byref(f), C.byref(s), C.byref(t), int(pdi), n, nsteps, arr,
                                         cf.ctypes.data_as(C.POINTER(C.c_double)), outs)
    for i in range(n):
        C.memmove(C.byref(chans[i]), C.byref(arr[i]), C.sizeof(abi.GnssVtChan))
    rec = np.ctypeslib.as_array(outs).reshape(nsteps, n)
    out = {k: rec[k].copy() for k in rec.dtype.names}
    try:
        ctx.check(st)
    except abi.GnssError as e:
        e.records = out
        raise
    return out


def trackingVT_mc_step(file, signal, track, chans, codeFreq_new, pdi=1, *, ctx: Context | None = None):
    """One step of trackingVT_mc_run -> one dict per channel."""
    cf = np.ascontiguousarray(codeFreq_new, dtype=np.float64).reshape(1, -1)
    out = trackingVT_mc_run(file, signal, track, chans, cf, pdi, ctx=ctx)
    return [{k: out[k][0, i] for k in out} for i in range(len(chans))]


def trackingVT_POS_updated_multicorrelator(file, signal, track, cmn, solu, Acquired, cnslxyz, eph, sbf,
                                           TckResult_Eph, TckResultCT, navSolutionsCT, *,
                                           ctx: Context | None = None, ALPHA_=None, BETA_=None,
                                           nsteps: int | None = None, return_cn0: bool = False):
    """trackingVT_POS_updated_multicorrelator.m:1-609 -> (TckResultVT_mltCorr,
    navSolutionsVT_mltCorr[, CN0_VT]): the vector-tracking loop SDR_main.m runs for
    cmn.mltCorrON = [1 1] (gnss_tracking_vt_mc).

    Arguments, initialisation and outputs as trackingVT_POS_updated, except what the reference's
    file changes: 25 real replicas at Spacing = 0.6:-0.05:-0.6 correlated sample by sample
    (E / P / L = Spacing(3) / (13) / (23), a real early-late codeError), the EKF's
    prr_measured from carrFreq - signal.IF (:504), no msStartTckVT clamp (:97: an index past
    TckResultCT raises IndexError as MATLAB does), and TckResultVT_mltCorr(prn) also carries the
    50 tap sums under the reference's names (E_i_060 ... E_i_005, L_i005 ... L_i060 and the _q
    twins, :401-450; tap_i / tap_q hold them as nsteps x 25 in Spacing order).
    """
    R, sols, sv, nsteps = _vt_loop(file, signal, track, cmn, solu, Acquired, cnslxyz, eph, sbf, TckResult_Eph,
                                   TckResultCT, navSolutionsCT, ctx, ALPHA_, BETA_, nsteps, False,
                                   "gnss_tracking_vt_mc", abi.GnssVtMcOut)
    n = len(sv)
    entries = {}
    for i, p in enumerate(sv):
        e = SimpleNamespace(**{k: R[k][:, i].astype(np.float64) for k in VT_FIELDS})
        e.sv_vel = R["sv_vel"][:, i].copy()
        e.tap_i, e.tap_q = R["tap_i"][:, i].copy(), R["tap_q"][:, i].copy()
        _mc_tap_fields(e, R, i)
        for k in ("amplitude", "navi_data", "navi_dataL035"):
            setattr(e, k, np.zeros(nsteps))
        entries[p] = e
    nsol = _navsol_arrays(sols, nsteps, n)
    res = StructArray(entries)
    res.acf_orient = abi.ACF_ORIENT["trackingVT_POS_updated_multicorrelator"]  # (acf_fit reads it)
    if return_cn0:
        return res, nsol, _cn0_rows(R, nsteps, n)
    return res, nsol


# ---------------------------------------------------------------------------
# findPosSV.m and the positioning half of trackingCT_POS_updated.m: navSolutionsCT
# ---------------------------------------------------------------------------
def findPosSV(file, Acquired, eph):
    """findPosSV.m:17-38 -> nAcquired: Acquired's channels whose ephemeris(prn).updateflag is 1,
    in Acquired's order (SDR_main.m:59,76 then loads it back as nAcquired). The reference's
    return value is the PRN list, which is nAcquired.sv; its side file
    nAcquired_<fileName>_<skip>.mat (:42) is not written."""
    keep = [i for i, p in enumerate(np.atleast_1d(Acquired.sv))
            if int(getattr(_struct_of(eph, p), "updateflag", 0)) == 1]
    print("Satellites used for positioning: ")
    print(" ".join(f"{int(np.atleast_1d(Acquired.sv)[i]):02d}" for i in keep) + " \n")
    pick = lambda v, dt: np.array([np.atleast_1d(v)[i] for i in keep], dtype=dt)
    return SimpleNamespace(sv=pick(Acquired.sv, np.int64), SNR=pick(Acquired.SNR, np.float64),
                           Doppler=pick(Acquired.Doppler, np.float64), codedelay=pick(Acquired.codedelay, np.int64),
                           fineFreq=pick(Acquired.fineFreq, np.float64))


class NavSolCtBuffers:
    """Caller-allocated gnss_nav_sol_ct: `cap` rows of every navSolutionsCT field for n channels."""

    def __init__(self, n: int, cap: int):
        self.n, self.cap = int(n), max(int(cap), 1)
        o = abi.GnssNavSolCt()
        o.cap = self.cap
        self.arr = {}
        for f, w in abi.NAVSOL_CT_FIELDS:
            self.arr[f] = np.zeros((self.cap, w or self.n))
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.arr["Index"] = np.zeros(self.cap, dtype=np.int64)
        self.arr["index"] = np.zeros((self.cap, self.n), dtype=np.int64)
        self.arr["carrFreqMeas"] = np.zeros((self.cap, self.n))
        self.arr["iters"] = np.zeros(self.cap, dtype=np.int32)
        o.Index = self.arr["Index"].ctypes.data_as(C.POINTER(C.c_int64))
        o.index = self.arr["index"].ctypes.data_as(C.POINTER(C.c_int64))
        o.carrFreqMeas = self.arr["carrFreqMeas"].ctypes.data_as(C.POINTER(C.c_double))
        o.iters = self.arr["iters"].ctypes.data_as(C.POINTER(C.c_int32))
        self.c = o

    def result(self) -> SimpleNamespace:
        """navSolutionsCT (trackingCT_POS_updated.m:509-551): rows x n / 3 / 4 matrices, clkBias /
        clkDrift / localTime as vectors; plus Index (the tracking step of each row), index,
        carrFreqMeas and iters, which the reference's struct does not have."""
        rows = int(self.c.rows)
        out = SimpleNamespace()
        for f, w in abi.NAVSOL_CT_FIELDS:
            a = self.arr[f][:rows].copy()
            setattr(out, f, a[:, 0] if w == 1 else a)
        for f in ("Index", "index", "carrFreqMeas", "iters"):
            setattr(out, f, self.arr[f][:rows].copy())
        return out


def _ct_pos_cfg(file, signal, track, cmn, Acquired, cnslxyz, eph, sbf, solu, countinx, TckResult_Eph, sampleStartMea,
                mode, ALPHA_, BETA_):
    sv = [int(p) for p in np.atleast_1d(Acquired.sv)]
    n = len(sv)
    if n > abi.VT_MAX_CH:
        raise ValueError(f"positioning takes at most {abi.VT_MAX_CH} channels")
    modes = {"pos_updated": abi.CT_POS_UPDATED, "multicorr": abi.CT_POS_MULTICORR}
    if mode not in modes:
        raise ValueError("mode is 'pos_updated' or 'multicorr'")
    cfg = abi.GnssCtPosCfg()
    cfg.n, cfg.mode, cfg.dataType = n, modes[mode], int(file.dataType)
    cfg.msToProcessCT_1ms = int(track.msToProcessCT_1ms)
    cfg.pdi = int(getattr(track, "pdi", 1))
    cfg.navSolPeriod = float(solu.navSolPeriod)
    cfg.Fs, cfg.IF, cfg.codelength, cfg.ms = float(signal.Fs), float(signal.IF), float(signal.codelength), float(signal.ms)
    cfg.cSpeed, cfg.doy = float(cmn.cSpeed), float(cmn.doy)
    cfg.cnslxyz[:] = [float(x) for x in np.asarray(cnslxyz, dtype=np.float64).ravel()[:3]]
    cfg.ALPHA[:] = [float(x) for x in (ALPHA_ if ALPHA_ is not None else ALPHA)]
    cfg.BETA[:] = [float(x) for x in (BETA_ if BETA_ is not None else BETA)]
    cx = np.asarray(countinx).reshape(-1)
    for i, p in enumerate(sv):
        e = _struct_of(eph, p)
        cfg.countinx[i] = int(cx[i])  # by channel position (:29,183; quirk A.17)
        cfg.nav1[i] = int(_vec1(sbf.nav1, p))
        cfg.sfb1[i] = int(_first(e.sfb))
        cfg.TOW1[i] = _first(e.TOW)
        cfg.eph[i] = eph_sv(eph, p)
        if sampleStartMea is not None:  # max(sampleStart) + 1 given outright (:160)
            cfg.sampleStart[i] = int(sampleStartMea) - 1
        else:  # :156 (MATLAB's 1-based index; raises as MATLAB does past the end)
            k = cfg.nav1[i] + cfg.sfb1[i] * 20
            a = np.asarray(_struct_of(TckResult_Eph, p).absoluteSample).ravel()
            if k < 1:
                raise IndexError("TckResult_Eph(prn).absoluteSample(nav1 + sfb(1)*20): index below 1")
            cfg.sampleStart[i] = int(a[k - 1])
    return cfg, sv


def ct_positioning(TckResultCT, file, signal, track, cmn, Acquired, cnslxyz, eph, sbf, solu, *, countinx,
                   TckResult_Eph=None, sampleStartMea: int | None = None, mode: str = "pos_updated",
                   ctx: Context | None = None, ALPHA_=None, BETA_=None):
    """The positioning half of trackingCT_POS_updated.m (:147-171, :420-565; mode="pos_updated")
    or of trackingCT_POS_updated_multicorrelator.m (:446-590; mode="multicorr", track.pdi) as a
    pass over given tracking records -> navSolutionsCT (gnss_ct_pos_solve).

    TckResultCT is the StructArray of trackingCT_POS / trackingCT_POS_updated_multicorrelator (or
    any per-PRN structs with absoluteSample, remChip, codeFreq, carrFreq), or their raw
    TrackOutBuffers; DeviceTrackOutBuffers keep the records in HBM and only the measurement
    table crosses PCIe. sampleStartMea replaces TckResult_Eph (:156-160) when given. Host records
    need no GPU (ctx may stay None without one). MATLAB's errors -> GnssError (index = 0:
    EINDEX; fewer than 4 satellites: EARG); olspos.m's uncapped loop stops with ENOCONV.
    """
    if sampleStartMea is None and TckResult_Eph is None:
        raise ValueError("ct_positioning needs TckResult_Eph or sampleStartMea")
    cfg, sv = _ct_pos_cfg(file, signal, track, cmn, Acquired, cnslxyz, eph, sbf, solu, countinx, TckResult_Eph,
                          sampleStartMea, mode, ALPHA_, BETA_)
    n = len(sv)
    lib = abi.load()
    if isinstance(TckResultCT, TrackOutBuffers):
        rec = TckResultCT.c
        steps = int(TckResultCT.len[:n].min()) if n else 0
        if isinstance(TckResultCT, DeviceTrackOutBuffers):
            ctx = ctx or default_context()
            TckResultCT.sync_producer()
    else:
        series = [[np.asarray(getattr(_struct_of(TckResultCT, p), f), dtype=np.float64).ravel()
                   for f in ("absoluteSample", "remChip", "codeFreq", "carrFreq")] for p in sv]
        lens = np.array([min(len(x) for x in s) for s in series], dtype=np.int64)
        steps = int(lens.min()) if n else 0
        arr = np.zeros((n, abi.NFIELDS, max(int(lens.max()) if n else 1, 1)))
        for i, s in enumerate(series):
            for f, x in zip(("absoluteSample", "remChip", "codeFreq", "carrFreq"), s):
                arr[i, abi.FIELDS_POS.index(f), : lens[i]] = x[: lens[i]]
        rec = abi.GnssTrackOut()
        rec.max_len = arr.shape[2]
        rec.rec = arr.ctypes.data_as(C.POINTER(C.c_double))
        rec.len = lens.ctypes.data_as(C.POINTER(C.c_int64))
    buf = NavSolCtBuffers(n, steps)
    h = ctx.h if ctx is not None else None
    st = lib.gnss_ct_pos_solve(h, C.byref(cfg), C.byref(rec), C.byref(buf.c))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    return buf.result()


def trackingCT_POS_updated(file, signal, track, cmn, Acquired, TckResult_Eph, cnslxyz, eph, sbf, solu, *, countinx,
                           ctx: Context | None = None, device_records: bool = False, ALPHA_=None, BETA_=None):
    """trackingCT_POS_updated.m:1-573 -> (TckResultCT_pos, navSolutionsCT): the reference's
    signature plus the `countinx` it loads from countinx.mat (:29).

    The scalar loops run as in trackingCT_POS (gnss_tracking_ct_pos, track.ctPOS steps), then the
    positioning pass over their records (gnss_ct_pos_solve; positioning does not feed back into
    the loops). With device_records the records stay in HBM between the two calls and the
    measurement table alone crosses PCIe before TckResultCT_pos is downloaded for the return
    value. navSolutionsCT is what trackingVT_POS_updated takes. The side files of :573-574 are
    not written.
    """
    ctx = ctx or default_context()
    nsv = len(Acquired.sv)
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    t, k2 = to_c_track(track, None, None)
    a = to_c_acquired(Acquired)
    cx = np.ascontiguousarray(np.asarray(countinx).reshape(-1)[:nsv], dtype=np.int32)
    ctPOS = int(track.ctPOS)
    if device_records:
        buf = DeviceTrackOutBuffers(nsv, track, 0, device=f"cuda:{ctx.device}", ctPOS=ctPOS)
        buf.sync_producer()
    else:
        buf = TrackOutBuffers(nsv, track, 0, ctPOS=ctPOS)
    ctx.check(ctx.lib.gnss_tracking_ct_pos(ctx.h, C.byref(f), C.byref(s), C.byref(t), C.byref(a), ctPOS,
                                           cx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(buf.c)))
    nav = ct_positioning(buf, file, signal, track, cmn, Acquired, cnslxyz, eph, sbf, solu, countinx=cx,
                         TckResult_Eph=TckResult_Eph, ctx=ctx, ALPHA_=ALPHA_, BETA_=BETA_)
    hb = buf.host() if device_records else buf
    return build_tck_result(Acquired, hb, None, abi.FIELDS_POS), nav


# ---------------------------------------------------------------------------
# ACF/CalculateFeatures.m: the multipath / NLOS features of the 25-tap records
# ---------------------------------------------------------------------------
def _acf_pack(TckResults_multiCorr, prnList):
    """The per-PRN structs of a 25-tap loop packed into the gnss_track_out layout: taps
    [n][2][25][max_len] and the code discriminator in the DLLdiscri slot. The scalar loops'
    structs carry taps_i / taps_q (25 x steps) and DLLdiscri or codeError, the vector loop's
    (TckResultVT_mltCorr) tap_i / tap_q (steps x 25) and codeError."""
    chans = []
    for p in prnList:
        e = _struct_of(TckResults_multiCorr, p)
        if hasattr(e, "taps_i"):
            ti, tq = np.asarray(e.taps_i, dtype=np.float64), np.asarray(e.taps_q, dtype=np.float64)
        else:
            ti, tq = np.asarray(e.tap_i, dtype=np.float64).T, np.asarray(e.tap_q, dtype=np.float64).T
        d = np.asarray(e.DLLdiscri if hasattr(e, "DLLdiscri") else e.codeError, dtype=np.float64).ravel()
        if ti.shape[0] != abi.MC_TAPS or tq.shape != ti.shape or len(d) < ti.shape[1]:
            raise ValueError(f"PRN {p}: 25 taps of I and Q and a code discriminator per step")
        chans.append((ti, tq, d))
    n = len(chans)
    lens = np.array([c[0].shape[1] for c in chans], dtype=np.int64)
    max_len = max(int(lens.max()) if n else 1, 1)
    rec = np.zeros((n, abi.NFIELDS, max_len))
    taps = np.zeros((n, 2, abi.MC_TAPS, max_len))
    for i, (ti, tq, d) in enumerate(chans):
        taps[i, 0, :, : lens[i]], taps[i, 1, :, : lens[i]] = ti, tq
        rec[i, abi.FIELDS.index("DLLdiscri"), : lens[i]] = d[: lens[i]]
    o = abi.GnssTrackOut()
    o.max_len = max_len
    o.rec = rec.ctypes.data_as(C.POINTER(C.c_double))
    o.taps = taps.ctypes.data_as(C.POINTER(C.c_double))
    o.len = lens.ctypes.data_as(C.POINTER(C.c_int64))
    return o, (rec, taps, lens)


def _acf_records(records, prn, ctx, who):
    """The gnss_track_out a pass over 25-tap records reads, for the raw TrackOutBuffers of a loop
    (host or device) or the per-PRN structs: (rec, what keeps its arrays alive, lens, max_len,
    on_device, ctx)."""
    n = len(prn)
    on_device = isinstance(records, DeviceTrackOutBuffers)
    if isinstance(records, TrackOutBuffers):
        if records.taps is None or records.taps.shape[2] != abi.MC_TAPS or records.taps.shape[0] < n:
            raise ValueError(f"{who}: the records of a 25-tap loop, one channel per PRN")
        lens, max_len = records.len, records.max_len
        if on_device:
            rec, keep = records.c, records
            ctx = ctx or default_context()
            records.sync_producer()
        else:  # (a host copy of device buffers still carries their gnss_track_out: build it anew)
            keep = (np.ascontiguousarray(records.rec, dtype=np.float64),
                    np.ascontiguousarray(records.taps, dtype=np.float64),
                    np.ascontiguousarray(records.len, dtype=np.int64))
            rec = abi.GnssTrackOut()
            rec.max_len = max_len
            rec.rec = keep[0].ctypes.data_as(C.POINTER(C.c_double))
            rec.taps = keep[1].ctypes.data_as(C.POINTER(C.c_double))
            rec.len = keep[2].ctypes.data_as(C.POINTER(C.c_int64))
    else:
        rec, keep = _acf_pack(records, prn)
        lens, max_len = keep[2], rec.max_len
    return rec, keep, lens, max_len, on_device, ctx


def acf_features(records, prnList, eleList, *, ctx: Context | None = None, want_index: bool = False,
                 want_corr: bool = False, extended: bool = False, **params):
    """The features of ACF/CalculateFeatures.m per channel (gnss_acf_features): a namespace of
    prn, ele, windows [n] and, per name of abi.ACF_FIELDS, a list of n arrays (one value per
    100-ms window): meanMax, F1 = meanMax / expectedCorr(ele), F2 = -meanDelay, varDelay,
    meanCodeDisc, varCodeDisc.

    `records`: the raw TrackOutBuffers of a 25-tap loop (channel c is prnList[c]), or the per-PRN
    structs the loops return (looked up by PRN, packed on the host). DeviceTrackOutBuffers stay in
    HBM: the kernels read them where they lie and only the features come back. params: ind_start,
    numOverLap, corrSpacing, maxDelay, a (abi.ACF_DEFAULTS). want_index / want_corr add
    maxCorrInd [n][max_len] (1-based arg-max per row) and corr [n][25][max_len], numpy arrays for
    host records and torch tensors on the device for device records. Host records need no GPU.

    extended=True (gnss_acf_features_ext) adds, per name of abi.ACF_EXT_FIELDS, the features the
    script keeps behind comment marks: numMLC (F6, the mean number of interior local maxima of a
    row's 25 magnitudes), fftFreq and fftMag (F7 / F8, the largest line of an fft_n-point
    spectrum of the channel's last fft_hist meanMax values: a reflected ray's fading frequency
    and depth). Its params: fft_hist, fft_n, fft_fill (abi.ACF_EXT_DEFAULTS; fft_fill=1 takes only
    the windows that exist in place of the script's zero-filled history), and fs, the windows per
    second, by default 1000 / (numOverLap * pdi) with pdi = 1 (:172; 10 with the script's numbers).
    """
    ext_keys = set(abi.ACF_EXT_DEFAULTS) | {"fs", "pdi"}
    unknown = set(params) - set(abi.ACF_DEFAULTS) - (ext_keys if extended else set())
    if unknown:
        raise TypeError(f"acf_features: unknown parameter(s) {sorted(unknown)}")
    xpar = dict(abi.ACF_EXT_DEFAULTS, **{k: params.pop(k) for k in list(params) if k in ext_keys})
    par = dict(abi.ACF_DEFAULTS, **params)
    prn = [int(p) for p in np.atleast_1d(prnList)]
    ele = [float(e) for e in np.atleast_1d(eleList)]
    n = len(prn)
    if len(ele) != n:
        raise ValueError("prnList and eleList differ in length")
    if n > abi.VT_MAX_CH:
        raise ValueError(f"acf_features takes at most {abi.VT_MAX_CH} channels")
    rec, keep, lens, max_len, on_device, ctx = _acf_records(records, prn, ctx, "acf_features")
    cfg = abi.GnssAcfCfg()
    cfg.n, cfg.ind_start, cfg.numOverLap = n, int(par["ind_start"]), int(par["numOverLap"])
    cfg.corrSpacing, cfg.maxDelay = float(par["corrSpacing"]), float(par["maxDelay"])
    cfg.a[:] = [float(x) for x in par["a"]]
    cfg.prn[:n], cfg.ele[:n] = prn, ele
    nov = max(cfg.numOverLap, 1)
    cap = max([max(int(l) - cfg.ind_start, 0) // nov for l in lens[:n]] + [1])
    out = abi.GnssAcfOut()
    out.cap = cap
    windows = np.zeros(max(n, 1), dtype=np.int64)
    out.windows = windows.ctypes.data_as(C.POINTER(C.c_int64))
    arr = {f: np.zeros((max(n, 1), cap)) for f in abi.ACF_FIELDS}
    for f in abi.ACF_FIELDS:
        setattr(out, f, arr[f].ctypes.data_as(C.POINTER(C.c_double)))
    ind = corr = None
    if on_device and (want_index or want_corr):
        import torch
        if want_index:
            ind = torch.zeros((n, max_len), dtype=torch.uint8, device=records.device)
            out.maxCorrInd = ind.data_ptr()
        if want_corr:
            corr = torch.zeros((n, abi.MC_TAPS, max_len), dtype=torch.float64, device=records.device)
            out.corr = corr.data_ptr()
        torch.cuda.current_stream(records.device).synchronize()
    elif want_index or want_corr:
        if want_index:
            ind = np.zeros((n, max_len), dtype=np.uint8)
            out.maxCorrInd = ind.ctypes.data
        if want_corr:
            corr = np.zeros((n, abi.MC_TAPS, max_len))
            out.corr = corr.ctypes.data
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    if extended:
        xcfg = abi.GnssAcfExtCfg()
        xcfg.fft_hist, xcfg.fft_n, xcfg.fft_fill = int(xpar["fft_hist"]), int(xpar["fft_n"]), int(xpar["fft_fill"])
        xcfg.fs = float(xpar["fs"]) if xpar.get("fs") is not None else 1000.0 / (nov * float(xpar.get("pdi", 1)))
        xout = abi.GnssAcfExtOut()
        for f in abi.ACF_EXT_FIELDS:
            arr[f] = np.zeros((max(n, 1), cap))
            setattr(xout, f, arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        st = lib.gnss_acf_features_ext(h, C.byref(cfg), C.byref(xcfg), C.byref(rec), abi.MC_TAPS, C.byref(out),
                                       C.byref(xout))
    else:
        st = lib.gnss_acf_features(h, C.byref(cfg), C.byref(rec), abi.MC_TAPS, C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    res = SimpleNamespace(prn=prn, ele=ele, windows=windows[:n].copy(), maxCorrInd=ind, corr=corr)
    for f in arr:
        setattr(res, f, [arr[f][c, : windows[c]].copy() for c in range(n)])
    return res


def CalculateFeatures(TckResults_multiCorr, prnList, eleList, *, ctx: Context | None = None,
                      extended: bool = False, **params):
    """ACF/CalculateFeatures.m:165-296 -> data_labeled, (1 + sum of the channels' windows) x 8:
    the script's all-zero first row (:165), then per PRN of prnList and per 100-ms window
    [prn, ele, meanMax, F1, F2, F3 = varDelay, F4 = meanCodeDisc, F5 = varCodeDisc] (:276-288).

    TckResults_multiCorr is what any of the three 25-tap loops returns (trackingCT_multiCorr,
    trackingCT_POS_updated_multicorrelator, trackingVT_POS_updated_multicorrelator) or their raw
    buffers, as for acf_features; prnList / eleList replace the script's hard-coded lists
    (:167-168) and params its hard-coded parameters (:172-179, :186). The plots of :298-323 are
    not drawn. extended=True: the 11-column form the script's data sets once had (:32), with
    F6 = numMLC, F7 = fftFreq, F8 = fftMag after F5 (acf_features' extended parameters)."""
    f = acf_features(TckResults_multiCorr, prnList, eleList, ctx=ctx, extended=extended, **params)
    fields = list(abi.ACF_FIELDS) + (list(abi.ACF_EXT_FIELDS) if extended else [])
    ncol = 2 + len(fields)
    rows = [np.zeros((1, ncol))]
    for c, (p, e) in enumerate(zip(f.prn, f.ele)):
        w = int(f.windows[c])
        rows.append(np.column_stack([np.full(w, float(p)), np.full(w, e)] +
                                    [getattr(f, k)[c] for k in fields]).reshape(w, ncol))
    return np.vstack(rows)


def acf_fit(records, prnList, *, ctx: Context | None = None, want_acf: bool = False, **params):
    """The two-path fit of the 25-tap ACF per feature window (gnss_acf_fit): a direct path plus
    one reflected path fitted to the window's coherently summed correlation function. A namespace
    of prn, windows [n] and, per name below, a list of n arrays with one value per window (the
    windows are acf_features': row m lines up with feature row m and label m):
      paths     2: the two-path model is selected, 1: one path, 0: no fit (a non-finite sum)
      bias      chips the prompt is late against the direct path (subtract it from the code
                delay); bias_m the same in metres, bias * cSpeed / codeFreqBasis
      p1, A1p_re, A1p_im, res1                     the one-path fit
      p0, e, A0_re, A0_im, A1_re, A1_im, res2      the two-path fit: the direct path at p0, the
                reflected one e chips later (NaN where no two-path hypothesis survived)
      ratio     |A1| / |A0|;  dphi_cycles  the reflected path's carrier phase against the direct
                path's, cycles in (-0.5, 0.5]
      energy    of the coherent vector; with want_acf also zI, zQ [25][windows] per channel.

    `records` as for acf_features; DeviceTrackOutBuffers are read where they lie by the kernel,
    host records need no GPU. params: orient (+1 / -1: which way the loop's Spacing runs over the
    stored taps; the three 25-tap loops tag what they return with it as .acf_orient, so it is
    needed only for records from elsewhere), ind_start, numOverLap, corrSpacing, the grid p_min,
    p_step, p_count, e_min, e_step, e_count, and ratio_max, gain_min (abi.ACF_FIT_DEFAULTS);
    cSpeed and codeFreqBasis for bias_m.
    """
    cSpeed = float(params.pop("cSpeed", 299792458.0))
    codeFreqBasis = float(params.pop("codeFreqBasis", 1.023e6))
    orient = params.pop("orient", getattr(records, "acf_orient", None))
    if orient is None:
        raise ValueError("acf_fit: orient (+1 or -1) is needed for records that no 25-tap loop tagged")
    unknown = set(params) - set(abi.ACF_FIT_DEFAULTS)
    if unknown:
        raise TypeError(f"acf_fit: unknown parameter(s) {sorted(unknown)}")
    par = dict(abi.ACF_FIT_DEFAULTS, **params)
    prn = [int(p) for p in np.atleast_1d(prnList)]
    n = len(prn)
    if n > abi.VT_MAX_CH:
        raise ValueError(f"acf_fit takes at most {abi.VT_MAX_CH} channels")
    rec, keep, lens, max_len, on_device, ctx = _acf_records(records, prn, ctx, "acf_fit")
    cfg = abi.GnssAcfFitCfg()
    cfg.n, cfg.orient = n, int(orient)
    for k in ("ind_start", "numOverLap", "p_count", "e_count"):
        setattr(cfg, k, int(par[k]))
    for k in ("corrSpacing", "p_min", "p_step", "e_min", "e_step", "ratio_max", "gain_min"):
        setattr(cfg, k, float(par[k]))
    nov = max(cfg.numOverLap, 1)
    cap = max([max(int(l) - cfg.ind_start, 0) // nov for l in lens[:n]] + [1])
    out = abi.GnssAcfFitOut()
    out.cap = cap
    windows = np.zeros(max(n, 1), dtype=np.int64)
    out.windows = windows.ctypes.data_as(C.POINTER(C.c_int64))
    paths = np.zeros((max(n, 1), cap), dtype=np.int32)
    out.paths = paths.ctypes.data_as(C.POINTER(C.c_int32))
    arr = {f: np.zeros((max(n, 1), cap)) for f in abi.ACF_FIT_FIELDS}
    if want_acf:
        arr["zI"], arr["zQ"] = np.zeros((max(n, 1), abi.MC_TAPS, cap)), np.zeros((max(n, 1), abi.MC_TAPS, cap))
    for f, a in arr.items():
        setattr(out, f, a.ctypes.data_as(C.POINTER(C.c_double)))
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    st = lib.gnss_acf_fit(h, C.byref(cfg), C.byref(rec), abi.MC_TAPS, C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    res = SimpleNamespace(prn=prn, windows=windows[:n].copy(), orient=int(orient),
                          paths=[paths[c, : windows[c]].copy() for c in range(n)])
    for f, a in arr.items():
        setattr(res, f, [a[c, ..., : windows[c]].copy() for c in range(n)])
    res.bias_m, res.ratio, res.dphi_cycles = [], [], []
    for c in range(n):
        a0 = res.A0_re[c] + 1j * res.A0_im[c]
        a1 = res.A1_re[c] + 1j * res.A1_im[c]
        with np.errstate(invalid="ignore", divide="ignore"):
            res.bias_m.append(res.bias[c] * cSpeed / codeFreqBasis)
            res.ratio.append(np.abs(a1) / np.abs(a0))
            res.dphi_cycles.append(np.angle(a1 * np.conj(a0)) / (2 * np.pi))
    return res


def scene_labels(scene, TckResults_multiCorr, prnList, *, ind_start: int = 1, numOverLap: int = 100,
                 bytes_per_sample: int = 2):
    """The ground truth of a synthetic scene (synth.scene_of / add_ray / set_nlos) for the feature
    windows of CalculateFeatures: per PRN of prnList an int array with one label per window,
      0  line of sight only,
      1  line of sight and at least one ray of that SV present at some sample of the window,
      2  no direct signal (los_gain == 0).
    Window m covers the records' rows ind_start - 1 + m*numOverLap ... + numOverLap - 1, as
    acf_features counts them. A row's samples come from absoluteSample, the file position after
    the row's read in bytes (int8 I/Q: bytes_per_sample = 2): row i spans
    [absoluteSample[i] - numSample[i]*bytes_per_sample, absoluteSample[i]). Host Python only."""
    out = []
    bps, N = int(bytes_per_sample), int(numOverLap)
    for p in np.atleast_1d(prnList):
        e = _struct_of(TckResults_multiCorr, p)
        pos = np.asarray(e.absoluteSample, dtype=np.float64).ravel().astype(np.int64)
        num = np.asarray(e.numSample, dtype=np.float64).ravel().astype(np.int64)
        L = len(pos)
        nwin = (L - ind_start) // N if L > ind_start else 0
        s = synth.sv_index(scene, int(p))
        rays = [scene.ray[r] for r in range(scene.n_ray) if scene.ray[r].sv == s and scene.ray[r].gain > 0 and scene.ray[r].t_off > scene.ray[r].t_on]
        lab = np.zeros(nwin, dtype=np.int64)
        for m in range(nwin):
            r0 = ind_start - 1 + m * N
            lo = (pos[r0] - num[r0] * bps) // bps  # first sample of the window
            hi = pos[r0 + N - 1] // bps            # one past its last
            if scene.los_gain[s] == 0:
                lab[m] = 2
            elif any(y.t_on < hi and y.t_off > lo for y in rays):
                lab[m] = 1
        out.append(lab)
    return out


# ---------------------------------------------------------------------------
# the classifier data_labeled is the training set of: k nearest neighbours over the feature windows
# ---------------------------------------------------------------------------
# feature_table's column names -> (which namespace, its field)
_KNN_COLUMNS = {"F1": ("features", "F1"), "F2": ("features", "F2"), "F3": ("features", "varDelay"),
                "F4": ("features", "meanCodeDisc"), "F5": ("features", "varCodeDisc"),
                "numMLC": ("features", "numMLC"), "fftFreq": ("features", "fftFreq"), "fftMag": ("features", "fftMag"),
                "bias": ("fit", "bias"), "ratio": ("fit", "ratio")}


def feature_table(features, fit=None, columns=None):
    """The [Q][D] table of an acf_features namespace and, if given, the acf_fit namespace of the
    same windows: one row per window, all channels concatenated in prnList order (which lines up
    with np.concatenate(scene_labels(...))). Default columns: F1, F2, F3 (varDelay), F4
    (meanCodeDisc), F5 (varCodeDisc), then numMLC, fftFreq, fftMag when the namespace is extended,
    then bias, ratio when `fit` is given. columns= selects by these names (any other per-window
    field of the two namespaces by its own name, e.g. "meanMax" or "e"); a name the inputs do not
    carry is a ValueError."""
    if columns is None:
        columns = ["F1", "F2", "F3", "F4", "F5"]
        if hasattr(features, "numMLC"):
            columns += ["numMLC", "fftFreq", "fftMag"]
        if fit is not None:
            columns += ["bias", "ratio"]
    src = {"features": features, "fit": fit}
    windows = [int(w) for w in features.windows]
    cols = []
    for name in columns:
        where, field = _KNN_COLUMNS.get(name, (None, name))
        holders = [src[where]] if where else [features, fit]
        per = next((getattr(h, field) for h in holders if h is not None and isinstance(getattr(h, field, None), list)),
                   None)
        if per is None or len(per) != len(windows) or any(np.shape(a) != (w,) for a, w in zip(per, windows)):
            raise ValueError(f"feature_table: the inputs carry no per-window column {name!r}")
        cols.append(np.concatenate([np.asarray(a, dtype=np.float64) for a in per]) if per else np.zeros(0))
    return np.column_stack(cols).reshape(sum(windows), len(cols)) if cols else np.zeros((sum(windows), 0))


def _knn_status(lib, h, st):
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode())


class KnnModel:
    """A trained k-NN model (knn_train): mu, inv [D], the standardised rows z [M][D], label [M],
    n_class, .dropped (the training rows left out for a non-finite value) and, trained with a
    context, z and label resident in its HBM until .free()."""

    def __init__(self, mu, inv, z, label, n_class, dropped, ctx=None):
        self.mu, self.inv, self.z, self.label = mu, inv, z, label
        self.n_class, self.dropped, self.ctx = int(n_class), int(dropped), None
        self.dev_z = self.dev_label = None
        if ctx is not None:
            lib = ctx.lib
            try:
                for name, a in (("dev_z", z), ("dev_label", label)):
                    p = C.c_void_p()
                    ctx.check(lib.gnss_dev_alloc(ctx.h, C.c_uint64(a.nbytes), C.byref(p)))
                    setattr(self, name, p)
                    ctx.check(lib.gnss_dev_upload(ctx.h, p, a.ctypes.data_as(C.c_void_p), C.c_uint64(a.nbytes)))
            except Exception:
                self.ctx = ctx
                self.free()
                raise
            self.ctx = ctx

    M = property(lambda self: self.z.shape[0])
    D = property(lambda self: self.z.shape[1])
    resident = property(lambda self: self.ctx is not None and self.dev_z is not None and self.dev_label is not None)

    def free(self):
        """Releases the resident copies (the host arrays stay: the model still classifies)."""
        if self.ctx is not None and getattr(self.ctx, "h", None):
            for p in (self.dev_z, self.dev_label):
                if p:
                    self.ctx.lib.gnss_dev_free(self.ctx.h, p)
        self.dev_z = self.dev_label = self.ctx = None

    def c_model(self, device: bool):
        m = abi.GnssKnnModel()
        m.M, m.D, m.n_class = self.M, self.D, self.n_class
        m.mu, m.inv = self.mu.ctypes.data, self.inv.ctypes.data
        if device:
            m.z, m.label, m.flags = self.dev_z.value, self.dev_label.value, abi.KNN_MODEL_DEVICE
        else:
            m.z, m.label = self.z.ctypes.data, self.label.ctypes.data
        return m


def knn_train(X, y, n_class: int = 3, ctx: Context | None = None) -> KnnModel:
    """A k-NN model of the table X [M][D] (feature_table) and its labels y [M] in 0..n_class-1
    (np.concatenate(scene_labels(...))). Rows with a non-finite value are dropped first and
    counted in .dropped; the columns are standardised by gnss_knn_standardize (a constant column
    drops out of every distance). With ctx the standardised rows and the labels are uploaded once
    and stay resident for knn_classify until .free(). Host work only otherwise."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y)
    if X.ndim != 2 or y.shape != (X.shape[0],):
        raise ValueError("knn_train: X [M][D] and y [M]")
    keep = np.all(np.isfinite(X), axis=1)
    dropped = int(np.sum(~keep))
    X, label = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep], dtype=np.int32)
    M, D = X.shape
    if M and not np.array_equal(label, y[keep]):
        raise ValueError("knn_train: y holds a value that is no 32-bit integer")
    if M and (label.min() < 0 or label.max() >= int(n_class)):
        raise ValueError(f"knn_train: a label outside 0..{int(n_class) - 1}")
    mu, inv, z = np.zeros(max(D, 1)), np.zeros(max(D, 1)), np.zeros((M, D))
    lib = abi.load()
    _knn_status(lib, None, lib.gnss_knn_standardize(X.ctypes.data, M, D, mu.ctypes.data, inv.ctypes.data,
                                                    z.ctypes.data))
    return KnnModel(mu[:D].copy(), inv[:D].copy(), z, label, n_class, dropped, ctx)


def knn_classify(model: KnnModel, X, k: int = 5, ctx: Context | None = None, want_neighbours: bool = False):
    """The rows of X [Q][D] labelled by the vote of their k nearest training rows
    (gnss_knn_classify): a namespace of label [Q] (-1 for a row with a non-finite value),
    votes [Q][n_class] and, with want_neighbours, nn_index [Q][k] (rows of the model's table after
    the dropped ones were taken out, nearest first) and nn_d2 [Q][k] (squared distances in
    standardised units). A resident model runs on its context's GPU; with ctx a host model is
    uploaded for the call; with neither the host path runs (no GPU needed). The three give the
    same bits."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != model.D:
        raise ValueError(f"knn_classify: X [Q][{model.D}]")
    if model.resident and ctx is not None and ctx is not model.ctx:
        raise ValueError("knn_classify: the model is resident on another context")
    run_ctx = model.ctx if model.resident else ctx
    Q, k = X.shape[0], int(k)
    cfg = abi.GnssKnnCfg()
    cfg.k = k
    cm = model.c_model(model.resident)
    kk = max(k, 1)
    res = SimpleNamespace(label=np.full(Q, -1, dtype=np.int32), votes=np.zeros((Q, model.n_class), dtype=np.int32))
    out = abi.GnssKnnOut()
    out.label, out.votes = res.label.ctypes.data, res.votes.ctypes.data
    if want_neighbours:
        res.nn_index, res.nn_d2 = np.full((Q, kk), -1, dtype=np.int32), np.full((Q, kk), np.nan)
        out.nn_index, out.nn_d2 = res.nn_index.ctypes.data, res.nn_d2.ctypes.data
    lib = abi.load()
    h = run_ctx.h if run_ctx is not None else None
    _knn_status(lib, h, lib.gnss_knn_classify(h, C.byref(cfg), C.byref(cm), X.ctypes.data, Q, C.byref(out)))
    return res


def confusion(y_true, y_pred, n_class: int = 3) -> np.ndarray:
    """[n_class][n_class + 1] counts: row = the true class, column = the predicted one, the last
    column the rows that got no label (-1)."""
    yt, yp = np.asarray(y_true).astype(np.int64).ravel(), np.asarray(y_pred).astype(np.int64).ravel()
    if yt.shape != yp.shape:
        raise ValueError("confusion: y_true and y_pred differ in length")
    if yt.size and (yt.min() < 0 or yt.max() >= n_class or yp.min() < -1 or yp.max() >= n_class):
        raise ValueError("confusion: a class outside 0..n_class-1 (or a prediction below -1)")
    m = np.zeros((n_class, n_class + 1), dtype=np.int64)
    np.add.at(m, (yt, np.where(yp < 0, n_class, yp)), 1)
    return m


# ---------------------------------------------------------------------------
# The replay correlator: recorded tracking rows on any tap grid (gnss_replay_correlate)
# ---------------------------------------------------------------------------
_REPLAY_SERIES = ("remChip", "codeFreq", "carrierFreq", "remPhase", "absoluteSample", "numSample")


def replay_rows(records, Acquired, file, signal, loop: str = "given", rows=None):
    """The replay table of a tracking result: per channel and row the NCO state its correlation
    started from. Row i of a loop reads numSample(i) samples from byte absoluteSample(i-1) with
    remChip, codeFreq, carrierFreq and remPhase as row i-1 left them; row 0 takes the loop's initial
    state (0, codeFreqBasis, fineFreq, 0) and its seek.

    `records`: the raw TrackOutBuffers (raw=True) of trackingCT_multiCorr (loop="given"),
    trackingCT_POS_updated_multicorrelator ("mc") or trackingCT_POS ("pos"); of device-resident
    records only those six series are downloaded. `rows`: the record rows to take, ascending
    indices applied to every channel (None: all of each channel). Returns a namespace with the
    table (prn, n_rows, max_rows, pos_bytes, numSample, remChip, codeFreq, carrFreq, remPhase
    [n_chan][max_rows]), rows (the record row of each table row), and what replays the loop's own
    correlation: taps, chip_off and post (0 / none for "given", 1 / none for "mc", 0 /
    [0, 0.05, 0] on the E / P / L taps [0.5, 0, -0.5] for "pos")."""
    if loop not in ("given", "mc", "pos"):
        raise ValueError('replay_rows: loop is "given", "mc" or "pos"')
    if not isinstance(records, TrackOutBuffers):
        raise ValueError("replay_rows: the raw TrackOutBuffers of a tracking loop (raw=True)")
    nch = len(Acquired.sv)
    idx = [abi.FIELDS.index(f) for f in _REPLAY_SERIES]
    if isinstance(records, DeviceTrackOutBuffers):
        records.sync_producer()
        ser = records.rec[:nch, idx, :].cpu().numpy()
    else:
        ser = np.asarray(records.rec)[:nch][:, idx, :]
    lens = [int(x) for x in np.asarray(records.len)[:nch]]
    S, skip = int(signal.Sample), int(file.skip)
    bps = int(file.dataPrecision) * int(file.dataType)
    sel = None if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    if sel is not None and len(sel) and (np.any(sel < 0) or np.any(np.diff(sel) <= 0)):
        raise ValueError("replay_rows: rows are ascending record row indices")
    per = [np.arange(n) if sel is None else sel[sel < n] for n in lens]
    max_rows = max([len(p) for p in per] + [1])
    t = SimpleNamespace(prn=np.array([int(p) for p in Acquired.sv], dtype=np.int32),
                        n_rows=np.array([len(p) for p in per], dtype=np.int64), max_rows=max_rows,
                        pos_bytes=np.zeros((nch, max_rows), dtype=np.int64),
                        numSample=np.zeros((nch, max_rows), dtype=np.int64),
                        remChip=np.zeros((nch, max_rows)), codeFreq=np.zeros((nch, max_rows)),
                        carrFreq=np.zeros((nch, max_rows)), remPhase=np.zeros((nch, max_rows)),
                        rows=per, loop=loop)
    for c in range(nch):
        cd = int(Acquired.codedelay[c])
        if loop == "given":  # trackingCT_multiCorr-GIVEN.m:57
            seek = (S - cd - 1 + skip * S) * bps
        else:                # trackingCT_POS_updated(_multicorrelator).m:108-110
            seek = int((S - cd + 1 + skip * signal.Fs * signal.ms) * bps)
        # the state before each row: the initial one, then every row's record
        start = np.empty((5, lens[c] + 1))
        start[:, 0] = [0.0, signal.codeFreqBasis, float(Acquired.fineFreq[c]), 0.0, float(seek)]
        start[:, 1:] = ser[c, :5, : lens[c]]
        r = per[c]
        k = len(r)
        t.remChip[c, :k], t.codeFreq[c, :k] = start[0, r], start[1, r]
        t.carrFreq[c, :k], t.remPhase[c, :k] = start[2, r], start[3, r]
        t.pos_bytes[c, :k] = np.rint(start[4, r]).astype(np.int64)
        t.numSample[c, :k] = np.rint(ser[c, 5, r]).astype(np.int64)
    spacing = colon(0.6, -0.05, -0.6)
    if loop == "given":
        t.taps, t.chip_off, t.post = colon(-0.6, 0.05, 0.6), 0, None
    elif loop == "mc":
        t.taps, t.chip_off, t.post = spacing, 1, None
    else:
        t.taps, t.chip_off, t.post = spacing[[2, 12, 22]], 0, np.array([0.0, 0.05, 0.0])
    return t


def replay_correlate(file, signal, rows, taps, chip_off: int = 0, post=None, ctx: Context | None = None,
                     device_out: bool = False):
    """Every tap's (I, Q) sum of every row of a replay table (replay_rows, or any namespace with
    its arrays) -> (taps_out, kernel_ms): taps_out [n_chan, 2, n_taps, max_rows] (I then Q, the
    layout of gnss_track_out.taps; rows beyond a channel's n_rows stay 0). `taps`: up to 256
    offsets in chips (a tap delays the replica: a ray tau chips late shows at tap -tau);
    chip_off / post as replay_rows returns them for the loop. ctx=None runs the host path (no
    GPU needed), a Context the kernel; device_out=True returns a torch tensor on the context's
    device (GNSS_OUT_DEVICE) instead of a numpy array."""
    f, k1 = to_c_file(file)
    s = to_c_signal(signal)
    tp = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    cfg = abi.GnssReplayCfg()
    cfg.n_taps, cfg.chip_off = len(tp), int(chip_off)
    cfg.tap_offsets = tp.ctypes.data
    if post is not None:
        po = np.ascontiguousarray(post, dtype=np.float64).reshape(-1)
        if len(po) != len(tp):
            raise ValueError("replay_correlate: post has one value per tap")
        cfg.post = po.ctypes.data
    nch, max_rows = len(rows.prn), int(rows.max_rows)
    keep = {"prn": np.ascontiguousarray(rows.prn, dtype=np.int32), "n_rows": np.ascontiguousarray(rows.n_rows, dtype=np.int64)}
    for name, dt in (("pos_bytes", np.int64), ("numSample", np.int64), ("remChip", np.float64),
                     ("codeFreq", np.float64), ("carrFreq", np.float64), ("remPhase", np.float64)):
        a = np.ascontiguousarray(getattr(rows, name), dtype=dt)
        if a.shape != (nch, max_rows):
            raise ValueError(f"replay_correlate: rows.{name} is not [n_chan][max_rows]")
        keep[name] = a
    r = abi.GnssReplayRows()
    r.n_chan, r.max_rows = nch, max_rows
    for name, a in keep.items():
        setattr(r, name, a.ctypes.data)
    out = abi.GnssReplayOut()
    if device_out:
        if ctx is None:
            raise ValueError("replay_correlate: device_out needs a Context")
        torch = abi.require_torch()
        res = torch.zeros((nch, 2, len(tp), max_rows), dtype=torch.float64, device=f"cuda:{ctx.device}")
        torch.cuda.current_stream(res.device).synchronize()
        out.taps = res.data_ptr()
        cfg.flags = abi.OUT_DEVICE
    else:
        res = np.zeros((nch, 2, len(tp), max_rows))
        out.taps = res.ctypes.data
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    st = lib.gnss_replay_correlate(h, C.byref(f), C.byref(s), C.byref(cfg), C.byref(r), C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    return res, float(out.kernel_ms)


def replay_coherent(taps_out, prompt, rows_per_window: int):
    """Each window's rows summed per tap with the sign of the prompt's I (the data-bit wipe of
    acf_fit, in numpy). taps_out [n_chan, 2, n_taps, n_rows] (replay_correlate's, cut to the
    rows wanted), prompt [n_chan, n_rows] the prompt's I of the same rows ->
    [n_chan, 2, n_taps, n_rows // rows_per_window]."""
    t = np.asarray(taps_out, dtype=np.float64)
    p = np.asarray(prompt, dtype=np.float64)
    w = int(rows_per_window)
    nwin = t.shape[3] // w
    sign = np.where(p[:, : nwin * w] < 0, -1.0, 1.0)
    z = t[:, :, :, : nwin * w] * sign[:, None, None, :]
    return z.reshape(t.shape[0], 2, t.shape[2], nwin, w).sum(axis=4)


# ---------------------------------------------------------------------------
# The two-path fit on any tap grid, fed by the replay (gnss_acf_fit_taps)
# ---------------------------------------------------------------------------
def acf_fit_taps(taps_out, n_rows, u, prompt=None, *, ctx: Context | None = None, want_acf: bool = False, **params):
    """acf_fit's two-path fit for sums on any tap grid (gnss_acf_fit_taps): per window of
    numOverLap rows a direct path plus one reflected path fitted to the coherently summed
    correlation function at the coordinates `u`. Returns acf_fit's namespace without prn and
    orient: windows [n] and, per name, a list of n arrays with one value per window -- paths, bias,
    bias_m, p1, A1p_re, A1p_im, res1, p0, e, A0_re, A0_im, A1_re, A1_im, res2, ratio, dphi_cycles,
    energy, with want_acf also zI, zQ [n_taps][windows] per channel -- plus u, prompt and
    kernel_ms (0 on the host path).

    `taps_out` [n, 2, n_taps, max_rows] as replay_correlate returns it: a numpy array (the host
    path, no GPU needed) or a torch tensor on the context's device, read where it lies by the
    kernel (device_out=True: only the fit rows leave HBM). `n_rows` [n]: the rows of each channel.
    `u` [n_taps]: the taps' coordinates in chips, a later path at a lower u; for replayed sums the
    tap offsets as they are. `prompt`: the index of the tap whose I gives a row's sign; None takes
    the one tap with u == 0. params: ind_start, numOverLap, the grid p_min, p_step, p_count, e_min,
    e_step, e_count, and ratio_max, gain_min (abi.ACF_FIT_TAPS_DEFAULTS); cSpeed and
    codeFreqBasis for bias_m."""
    cSpeed = float(params.pop("cSpeed", 299792458.0))
    codeFreqBasis = float(params.pop("codeFreqBasis", 1.023e6))
    unknown = set(params) - set(abi.ACF_FIT_TAPS_DEFAULTS)
    if unknown:
        raise TypeError(f"acf_fit_taps: unknown parameter(s) {sorted(unknown)}")
    par = dict(abi.ACF_FIT_TAPS_DEFAULTS, **params)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    nt = len(uu)
    if prompt is None:
        zero = np.flatnonzero(uu == 0)
        if len(zero) != 1:
            raise ValueError(f"acf_fit_taps: {len(zero)} taps have u == 0; name the prompt tap")
        prompt = int(zero[0])
    on_device = hasattr(taps_out, "data_ptr")
    if on_device:
        if ctx is None:
            raise ValueError("acf_fit_taps: a device tensor needs a Context")
        torch = abi.require_torch()
        t = taps_out
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.device.index != ctx.device:
            raise ValueError("acf_fit_taps: the tensor is contiguous float64 on the context's device")
        torch.cuda.current_stream(t.device).synchronize()
        ptr = t.data_ptr()
    else:
        t = np.ascontiguousarray(taps_out, dtype=np.float64)
        ptr = t.ctypes.data
    if t.ndim != 4 or t.shape[1] != 2 or t.shape[2] != nt:
        raise ValueError("acf_fit_taps: taps_out is [n, 2, n_taps, max_rows] with one u per tap")
    n, max_rows = int(t.shape[0]), int(t.shape[3])
    if n > abi.VT_MAX_CH:
        raise ValueError(f"acf_fit_taps takes at most {abi.VT_MAX_CH} channels")
    nr = np.ascontiguousarray(n_rows, dtype=np.int64).reshape(-1)
    if len(nr) != n:
        raise ValueError("acf_fit_taps: n_rows has one value per channel")
    cfg = abi.GnssAcfFitTapsCfg()
    cfg.n, cfg.n_taps, cfg.prompt = n, nt, int(prompt)
    cfg.u = uu.ctypes.data
    cfg.flags = abi.OUT_DEVICE if on_device else 0
    for k in ("ind_start", "numOverLap", "p_count", "e_count"):
        setattr(cfg, k, int(par[k]))
    for k in ("p_min", "p_step", "e_min", "e_step", "ratio_max", "gain_min"):
        setattr(cfg, k, float(par[k]))
    src = abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = ptr, max_rows, nr.ctypes.data
    nov = max(cfg.numOverLap, 1)
    cap = max([max(int(l) - cfg.ind_start, 0) // nov for l in nr] + [1])
    out = abi.GnssAcfFitOut()
    out.cap = cap
    windows = np.zeros(max(n, 1), dtype=np.int64)
    out.windows = windows.ctypes.data_as(C.POINTER(C.c_int64))
    paths = np.zeros((max(n, 1), cap), dtype=np.int32)
    out.paths = paths.ctypes.data_as(C.POINTER(C.c_int32))
    arr = {f: np.zeros((max(n, 1), cap)) for f in abi.ACF_FIT_FIELDS}
    if want_acf:
        arr["zI"], arr["zQ"] = np.zeros((max(n, 1), nt, cap)), np.zeros((max(n, 1), nt, cap))
    for f, a in arr.items():
        setattr(out, f, a.ctypes.data_as(C.POINTER(C.c_double)))
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    st = lib.gnss_acf_fit_taps(h, C.byref(cfg), C.byref(src), C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    res = SimpleNamespace(windows=windows[:n].copy(), u=uu, prompt=int(prompt),
                          kernel_ms=float(ctx.timing()["track_kernel_ms"]) if on_device else 0.0,
                          paths=[paths[c, : windows[c]].copy() for c in range(n)])
    for f, a in arr.items():
        setattr(res, f, [a[c, ..., : windows[c]].copy() for c in range(n)])
    res.bias_m, res.ratio, res.dphi_cycles = [], [], []
    for c in range(n):
        a0 = res.A0_re[c] + 1j * res.A0_im[c]
        a1 = res.A1_re[c] + 1j * res.A1_im[c]
        with np.errstate(invalid="ignore", divide="ignore"):
            res.bias_m.append(res.bias[c] * cSpeed / codeFreqBasis)
            res.ratio.append(np.abs(a1) / np.abs(a0))
            res.dphi_cycles.append(np.angle(a1 * np.conj(a0)) / (2 * np.pi))
    return res


def replay_fit(file, signal, rows, taps, *, chip_off: int = 0, post=None, ctx: Context | None = None, **params):
    """replay_correlate on `taps`, then acf_fit_taps with u = taps on the replayed sums: the
    multipath delay estimate on a grid of the caller's choice (a ray more than 0.6 chip late is in
    none of the 25-tap records). With a Context both steps run on the GPU and the sums stay in
    HBM between them (GNSS_OUT_DEVICE): only the fit rows come back. Returns acf_fit_taps'
    namespace with kernel_ms = (the replay's, the fit's). params: acf_fit_taps' (prompt, want_acf,
    the windows, the grid and the thresholds)."""
    tp = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    sums, replay_ms = replay_correlate(file, signal, rows, tp, chip_off=chip_off, post=post, ctx=ctx,
                                       device_out=ctx is not None)
    res = acf_fit_taps(sums, rows.n_rows, tp, params.pop("prompt", None), ctx=ctx, **params)
    res.kernel_ms = (float(replay_ms), res.kernel_ms)
    return res


# ---------------------------------------------------------------------------
# The multi-ray fit on any tap grid (gnss_acf_fit_multi)
# ---------------------------------------------------------------------------
def acf_fit_multi(taps_out, n_rows, u, prompt=None, *, ctx: Context | None = None, want_acf: bool = False, **params):
    """Up to four paths (the direct one and up to three rays) fitted to each window's coherently
    summed correlation function at the coordinates `u` (gnss_acf_fit_multi): alternating
    projection, a path's position searched on the grid q while the others stay, all amplitudes
    solved jointly. Returns a namespace: windows [n] and, per name, a list of n arrays -- paths,
    searches, bias, bias_m, energy [windows]; q, A_re, A_im, ratio, dphi_cycles, e [4][windows] (the
    selected order's paths, the earliest arrival first, NaN beyond `paths`; ratio[k] = |A_k|/|A_0|,
    dphi_cycles[k] the phase of A_k against A_0, e[k] = q[0] - q[k], the delay after the first
    path); res [5][windows] (res[0] = energy, res[m] order m's residual, NaN if not formed); with
    want_acf also zI, zQ [n_taps][windows] -- plus u, prompt and kernel_ms (0 on the host path).

    `taps_out`, `n_rows`, `u`, `prompt`, `ctx`: as acf_fit_taps (a numpy array runs the host path, a
    torch tensor on the context's device the kernel, which reads the sums where they lie). params:
    ind_start, numOverLap, q_min, q_step, q_count, max_paths, sweeps, sep_min, gain_min
    (abi.ACF_FIT_MULTI_DEFAULTS); cSpeed and codeFreqBasis for bias_m."""
    cSpeed = float(params.pop("cSpeed", 299792458.0))
    codeFreqBasis = float(params.pop("codeFreqBasis", 1.023e6))
    unknown = set(params) - set(abi.ACF_FIT_MULTI_DEFAULTS)
    if unknown:
        raise TypeError(f"acf_fit_multi: unknown parameter(s) {sorted(unknown)}")
    par = dict(abi.ACF_FIT_MULTI_DEFAULTS, **params)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    nt = len(uu)
    if prompt is None:
        zero = np.flatnonzero(uu == 0)
        if len(zero) != 1:
            raise ValueError(f"acf_fit_multi: {len(zero)} taps have u == 0; name the prompt tap")
        prompt = int(zero[0])
    on_device = hasattr(taps_out, "data_ptr")
    if on_device:
        if ctx is None:
            raise ValueError("acf_fit_multi: a device tensor needs a Context")
        torch = abi.require_torch()
        t = taps_out
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.device.index != ctx.device:
            raise ValueError("acf_fit_multi: the tensor is contiguous float64 on the context's device")
        torch.cuda.current_stream(t.device).synchronize()
        ptr = t.data_ptr()
    else:
        t = np.ascontiguousarray(taps_out, dtype=np.float64)
        ptr = t.ctypes.data
    if t.ndim != 4 or t.shape[1] != 2 or t.shape[2] != nt:
        raise ValueError("acf_fit_multi: taps_out is [n, 2, n_taps, max_rows] with one u per tap")
    n, max_rows = int(t.shape[0]), int(t.shape[3])
    if n > abi.VT_MAX_CH:
        raise ValueError(f"acf_fit_multi takes at most {abi.VT_MAX_CH} channels")
    nr = np.ascontiguousarray(n_rows, dtype=np.int64).reshape(-1)
    if len(nr) != n:
        raise ValueError("acf_fit_multi: n_rows has one value per channel")
    cfg = abi.GnssAcfFitMultiCfg()
    cfg.n, cfg.n_taps, cfg.prompt = n, nt, int(prompt)
    cfg.u = uu.ctypes.data
    cfg.flags = abi.OUT_DEVICE if on_device else 0
    for k in ("ind_start", "numOverLap", "q_count", "max_paths", "sweeps", "sep_min"):
        setattr(cfg, k, int(par[k]))
    for k in ("q_min", "q_step", "gain_min"):
        setattr(cfg, k, float(par[k]))
    src = abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = ptr, max_rows, nr.ctypes.data
    nov = max(cfg.numOverLap, 1)
    cap = max([max(int(l) - cfg.ind_start, 0) // nov for l in nr] + [1])
    P, nn = abi.ACF_MULTI_MAX_PATHS, max(n, 1)
    out = abi.GnssAcfFitMultiOut()
    out.cap = cap
    windows = np.zeros(nn, dtype=np.int64)
    out.windows = windows.ctypes.data_as(C.POINTER(C.c_int64))
    ints = {f: np.zeros((nn, cap), dtype=np.int32) for f in ("paths", "searches")}
    for f, a in ints.items():
        setattr(out, f, a.ctypes.data_as(C.POINTER(C.c_int32)))
    arr = {"bias": np.zeros((nn, cap)), "energy": np.zeros((nn, cap)), "res": np.zeros((nn, P + 1, cap))}
    arr.update({f: np.zeros((nn, P, cap)) for f in ("q", "A_re", "A_im")})
    if want_acf:
        arr["zI"], arr["zQ"] = np.zeros((nn, nt, cap)), np.zeros((nn, nt, cap))
    for f, a in arr.items():
        setattr(out, f, a.ctypes.data_as(C.POINTER(C.c_double)))
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    st = lib.gnss_acf_fit_multi(h, C.byref(cfg), C.byref(src), C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    res = SimpleNamespace(windows=windows[:n].copy(), u=uu, prompt=int(prompt),
                          kernel_ms=float(ctx.timing()["track_kernel_ms"]) if on_device else 0.0)
    for f, a in {**ints, **arr}.items():
        setattr(res, f, [a[c, ..., : windows[c]].copy() for c in range(n)])
    res.bias_m, res.ratio, res.dphi_cycles, res.e = [], [], [], []
    for c in range(n):
        a = res.A_re[c] + 1j * res.A_im[c]
        with np.errstate(invalid="ignore", divide="ignore"):
            res.bias_m.append(res.bias[c] * cSpeed / codeFreqBasis)
            res.ratio.append(np.abs(a) / np.abs(a[0]))
            res.dphi_cycles.append(np.angle(a * np.conj(a[0])) / (2 * np.pi))
            res.e.append(res.q[c][0] - res.q[c])
    return res


def replay_fit_multi(file, signal, rows, taps, *, chip_off: int = 0, post=None, ctx: Context | None = None, **params):
    """replay_correlate on `taps`, then acf_fit_multi with u = taps on the replayed sums: several
    rays on a grid of the caller's choice. With a Context both steps run on the GPU and the sums
    stay in HBM between them (GNSS_OUT_DEVICE): only the fit rows come back. Returns acf_fit_multi's
    namespace with kernel_ms = (the replay's, the fit's). params: acf_fit_multi's (prompt, want_acf,
    the windows, the grid and the search parameters)."""
    tp = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    sums, replay_ms = replay_correlate(file, signal, rows, tp, chip_off=chip_off, post=post, ctx=ctx,
                                       device_out=ctx is not None)
    res = acf_fit_multi(sums, rows.n_rows, tp, params.pop("prompt", None), ctx=ctx, **params)
    res.kernel_ms = (float(replay_ms), res.kernel_ms)
    return res


# ---------------------------------------------------------------------------
# The delay-Doppler map over replayed rows (gnss_replay_ddm)
# ---------------------------------------------------------------------------
def replay_ddm(taps_out, rows, dopp_hz, *, u, prompt, rows_per_window: int, signal, file, ctx: Context | None = None,
               want_map: bool = True, device_out: bool = False, excl_chips: float = 0.3, excl_hz: float = 10.0):
    """The delay-Doppler map of every window of rows_per_window consecutive rows of a replay: per
    tap and per Doppler offset the window's rows summed coherently with one rotation per row, held
    at the row's middle sample -- the correlation the loop would have seen with its carrier
    dopp_hz[m] higher (gnss_replay_ddm). A reflected ray with a carrier offset (synth.add_ray's
    fade_hz) cancels in replay_coherent's zero-offset sum; here it stands at (its delay, its
    offset), with the sign.

    `taps_out` [n, 2, n_taps, max_rows] as replay_correlate returns it: a numpy array (the host
    path, no GPU needed) or a torch tensor on the context's device, read where it lies by the
    kernel. `rows`: the replay table the sums came from (n_rows, pos_bytes, numSample: the rows'
    times). `u` [n_taps]: the taps' coordinates in chips (for replayed sums the tap offsets);
    `prompt`: the tap whose I gives a row's sign, None for the one tap with u == 0, -1 for no sign
    wipe. excl_chips / excl_hz: the secondary peak is the largest cell at least excl_chips OR at
    least excl_hz away from the peak.

    Returns a namespace: n_win [n]; per name a list of n arrays with one value per window --
    peak_tap, peak_bin, peak_chips, peak_hz, peak_pow, sec_tap, sec_bin, sec_chips, sec_hz, sec_pow
    (-1 / NaN where there is none); map, with want_map a list of n arrays [n_win, 2, n_dopp,
    n_taps] (ZI then ZQ), or with device_out one torch tensor [n, cap, 2, n_dopp, n_taps] that
    never left the device; u, dopp_hz, prompt and kernel_ms (0 on the host path)."""
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    hz = np.ascontiguousarray(dopp_hz, dtype=np.float64).reshape(-1)
    nt, nd = len(uu), len(hz)
    if prompt is None:
        zero = np.flatnonzero(uu == 0)
        if len(zero) != 1:
            raise ValueError(f"replay_ddm: {len(zero)} taps have u == 0; name the prompt tap")
        prompt = int(zero[0])
    on_device = hasattr(taps_out, "data_ptr")
    if device_out and not on_device:
        raise ValueError("replay_ddm: device_out needs device sums (a torch tensor) and a Context")
    if on_device:
        if ctx is None:
            raise ValueError("replay_ddm: a device tensor needs a Context")
        torch = abi.require_torch()
        t = taps_out
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.device.index != ctx.device:
            raise ValueError("replay_ddm: the tensor is contiguous float64 on the context's device")
        torch.cuda.current_stream(t.device).synchronize()
        ptr = t.data_ptr()
    else:
        t = np.ascontiguousarray(taps_out, dtype=np.float64)
        ptr = t.ctypes.data
    if t.ndim != 4 or t.shape[1] != 2 or t.shape[2] != nt:
        raise ValueError("replay_ddm: taps_out is [n, 2, n_taps, max_rows] with one u per tap")
    n, max_rows = int(t.shape[0]), int(t.shape[3])
    nr = np.ascontiguousarray(rows.n_rows, dtype=np.int64).reshape(-1)
    pos = np.ascontiguousarray(rows.pos_bytes, dtype=np.int64)
    ns = np.ascontiguousarray(rows.numSample, dtype=np.int64)
    if len(nr) != n or pos.shape != (n, max_rows) or ns.shape != (n, max_rows):
        raise ValueError("replay_ddm: rows.n_rows is [n], rows.pos_bytes and rows.numSample are [n][max_rows]")
    cfg = abi.GnssReplayDdmCfg()
    cfg.n, cfg.n_taps, cfg.prompt, cfg.rows_per_window, cfg.n_dopp = n, nt, int(prompt), int(rows_per_window), nd
    cfg.dopp_hz, cfg.u = hz.ctypes.data, uu.ctypes.data
    cfg.excl_chips, cfg.excl_hz, cfg.Fs = float(excl_chips), float(excl_hz), float(signal.Fs)
    cfg.bytes_per_sample = int(file.dataPrecision) * int(file.dataType)
    cfg.flags = (abi.OUT_DEVICE if on_device else 0) | (abi.DDM_MAP_DEVICE if device_out else 0)
    src = abi.GnssReplayDdmIn()
    src.taps, src.max_rows = ptr, max_rows
    src.n_rows, src.pos_bytes, src.numSample = nr.ctypes.data, pos.ctypes.data, ns.ctypes.data
    cap = max([int(k) // max(cfg.rows_per_window, 1) for k in nr] + [1])
    out = abi.GnssReplayDdmOut()
    out.cap = cap
    n_win = np.zeros(max(n, 1), dtype=np.int64)
    out.n_win = n_win.ctypes.data
    ints = {f: np.full((max(n, 1), cap), -1, dtype=np.int32) for f in ("peak_bin", "peak_tap", "sec_bin", "sec_tap")}
    pows = {f: np.full((max(n, 1), cap), np.nan) for f in ("peak_pow", "sec_pow")}
    for f, a in {**ints, **pows}.items():
        setattr(out, f, a.ctypes.data)
    m = None
    if device_out:
        m = torch.zeros((n, cap, 2, nd, nt), dtype=torch.float64, device=f"cuda:{ctx.device}")
        torch.cuda.current_stream(m.device).synchronize()
        out.map = m.data_ptr()
    elif want_map:
        m = np.zeros((max(n, 1), cap, 2, nd, nt))
        out.map = m.ctypes.data
    lib = abi.load()
    h = ctx.h if ctx is not None else None
    st = lib.gnss_replay_ddm(h, C.byref(cfg), C.byref(src), C.byref(out))
    if st != abi.OK:
        msg = (lib.gnss_last_error(h) or b"").decode() if h else lib.gnss_strerror(st).decode()
        raise abi.GnssError(st, msg)
    res = SimpleNamespace(n_win=n_win[:n].copy(), u=uu, dopp_hz=hz, prompt=int(prompt), kernel_ms=float(out.kernel_ms))
    for f, a in {**ints, **pows}.items():
        setattr(res, f, [a[c, : n_win[c]].copy() for c in range(n)])
    for who in ("peak", "sec"):
        tap, bin_ = getattr(res, who + "_tap"), getattr(res, who + "_bin")
        setattr(res, who + "_chips", [np.where(x >= 0, uu[np.maximum(x, 0)], np.nan) for x in tap])
        setattr(res, who + "_hz", [np.where(x >= 0, hz[np.maximum(x, 0)], np.nan) for x in bin_])
    res.map = m if device_out or m is None else [m[c, : n_win[c]].copy() for c in range(n)]
    return res
