/*
 * gnss_mi355x.h — C-ABI drop-in boundary for the GPS L1 C/A acquisition +
 * conventional-tracking hot path of KangWelly/Assignment-for-AAE6102_GNSS-SDR,
 * implemented with hand-written CDNA4 (gfx950) HIP kernels.
 *
 * The reference boundary is two MATLAB function calls (no FFI of its own):
 *
 *   Acquired = acquisition(file, signal, acq)
 *       SDR_MATLAB-main/acqtckpos/acquisition.m:1, called from SDR_main.m:22
 *       and Plot_task_1.m:14
 *   [TckResultCT, CN0_Eph, countinx] = trackingCT(file, signal, track, Acquired)
 *       SDR_MATLAB-main/acqtckpos/trackingCT.m:1, called from SDR_main.m:38
 *
 * The structs below carry exactly the MATLAB struct fields those functions read
 * (SDR_MATLAB-main/initParameters.m:20-70), as POD with fixed-width members.
 * Everything is plain pointers and sizes; no torch / HIP types cross this line.
 * The caller allocates every output; all lengths are known in advance.
 *
 * Threading: a gnss_ctx is bound to one HIP device and is not re-entrant
 * (MATLAB calls the MEX from one thread; the ctypes harness follows that rule).
 */
#ifndef GNSS_MI355X_H
#define GNSS_MI355X_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNSS_ABI_VERSION 14

/* ---- status codes (SURVEY §8b "Error conventions") --------------------- */
#define GNSS_OK         0
#define GNSS_ENODATA    1  /* reference's empty-result paths: "No satellites acquired"
                              (acquisition.m:84-85) / "Not enough raw data" ->
                              TckResultCT = [] (trackingCT.m:108-112, 302-306)          */
#define GNSS_EIO        2  /* file cannot be opened/read, or phase-C read past EOF
                              (trackingCT.m:442 has no check: MATLAB raises an error)  */
#define GNSS_EARG       3  /* bad/unsupported argument                                  */
#define GNSS_EDEVICE    4  /* HIP / rocFFT failure                                      */
#define GNSS_EINDEX     5  /* an index MATLAB would reject (e.g. P_i(i+17) past the end
                              in the bit-edge search, trackingCT.m:179-204)             */

#define GNSS_MAX_SV     64   /* generateCAcode.m:16-27 knows 51 PRNs                     */
#define GNSS_MAX_TAPS   32

/* ---- config structs (initParameters.m) ---------------------------------- */

/* file.* (initParameters.m:20-21,35-38). Exactly one of path / data / dev_data
 * is used, in that order of preference reversed (dev_data, then data, then
 * path). All seeks are absolute ('bof'), so positioned reads of `path` are
 * equivalent to MATLAB's fseek/fread on file.fid (SURVEY §8b "File handle"). */
typedef struct gnss_file {
    const char   *path;          /* file.fileRoute, or NULL                          */
    const int8_t *data;          /* host-resident IF record (byte 0 = file byte 0)   */
    const void   *dev_data;      /* IF record already resident in this ctx's HBM     */
    uint64_t      nbytes;        /* bytes in data / dev_data (ignored for path)      */
    int64_t       skip;          /* file.skip, ms                                    */
    int32_t       dataType;      /* file.dataType: 1 = I, 2 = IQ                     */
    int32_t       dataPrecision; /* file.dataPrecision: 1 = int8, 2 = int16          */
} gnss_file;

/* signal.* (initParameters.m:41-48) */
typedef struct gnss_signal {
    double  IF;              /* Hz                                  */
    double  Fs;              /* Hz                                  */
    double  codeFreqBasis;   /* 1.023e6                             */
    double  ms;              /* 1e-3                                */
    int64_t Sample;          /* ceil(Fs*ms)                         */
    double  codelength;      /* codeFreqBasis*ms                    */
} gnss_signal;

/* acq.* (initParameters.m:50-55) */
typedef struct gnss_acq {
    int32_t        freqNum;
    double         freqMin;
    double         freqStep;
    int32_t        datalen;   /* ms of non-coherent 1-ms FFT correlations            */
    int32_t        L;         /* ms used by the fine-frequency FFT                   */
    int32_t        n_prn;     /* 0 -> PRNs 1..32, as acquisition.m:47 hard-codes     */
    const int32_t *prn_list;  /* explicit PRN list (config 1: {3}; rank sharding)    */
} gnss_acq;

/* Acquired (acquisition.m:19-23,71-74,121): row vectors in ascending PRN order. */
typedef struct gnss_acquired {
    int32_t n;
    int32_t sv[GNSS_MAX_SV];
    double  SNR[GNSS_MAX_SV];
    double  Doppler[GNSS_MAX_SV];
    int32_t codedelay[GNSS_MAX_SV];
    double  fineFreq[GNSS_MAX_SV];
} gnss_acquired;

/* Per-PRN detector diagnostics (not part of the reference struct): every tested
 * PRN, acquired or not. peak2 = largest correlation value outside the peak's
 * +-56-sample exclusion window of the peak bin (margin of the argmax). */
typedef struct gnss_acq_diag {
    int32_t n;
    int32_t prn[GNSS_MAX_SV];
    double  SNR[GNSS_MAX_SV];
    int32_t fbin[GNSS_MAX_SV];        /* 1-based, as MATLAB                         */
    int32_t codePhase[GNSS_MAX_SV];   /* 1-based                                    */
    double  peak[GNSS_MAX_SV];
    double  peak2[GNSS_MAX_SV];
} gnss_acq_diag;

/* track.* (initParameters.m:58-70) */
typedef struct gnss_track {
    double  CorrelatorSpacing;      /* chip                                         */
    double  DLLBW, DLLDamp, DLLGain;
    double  PLLBW, PLLDamp, PLLGain;
    int32_t msToProcessCT_1ms;      /* the 1-ms phases A/B (trackingCT.m:29,221)    */
    int32_t msToProcessCT_10ms;     /* the 10-ms phase C (trackingCT.m:384)         */
    /* Multi-correlator ACF taps (config 5; semantics of
     * trackingCT_multiCorr-GIVEN.m:25,92-143). n_taps = 0 -> the three E/P/L taps
     * [-CorrelatorSpacing 0 +CorrelatorSpacing] (trackingCT.m:24). Otherwise
     * tap_offsets[n_taps] (chips) must contain -CorrelatorSpacing, 0 and
     * +CorrelatorSpacing, which feed the DLL/PLL exactly as E/P/L do. n_taps is
     * 3, 11 (config 5: -0.5:0.1:0.5) or 25 (-0.6:0.05:0.6 of the GIVEN file; int8
     * records only).                                                           */
    int32_t        n_taps;
    const double  *tap_offsets;
    /* Channel shard (multi-GPU): process Acquired channels chan[0..n_chan-1]
     * (0-based svindex) only; NULL -> every channel. Outputs of other channels
     * are left untouched. The quirk of trackingCT.m:161 (linear indexing into an
     * nsv x N matrix) uses the GLOBAL svindex and nsv, so shards stay bit-equal.  */
    int32_t        n_chan;
    const int32_t *chan;
} gnss_track;

/* Fields of one TckResultCT(prn) entry, in trackingCT.m:153-170 order. */
enum gnss_track_field {
    GNSS_F_P_i = 0, GNSS_F_P_q, GNSS_F_E_i, GNSS_F_E_q, GNSS_F_L_i, GNSS_F_L_q,
    GNSS_F_PLLdiscri, GNSS_F_DLLdiscri, GNSS_F_codedelay, GNSS_F_remChip,
    GNSS_F_codeFreq, GNSS_F_carrierFreq, GNSS_F_remPhase, GNSS_F_remSample,
    GNSS_F_numSample, GNSS_F_delayValue, GNSS_F_absoluteSample, GNSS_F_codedelay2,
    GNSS_NFIELDS
};

/* gnss_tracking_ct_pos stores trackingCT_POS_updated.m:273-292's fields in the same
 * slots: PLLdiscri = carrError, DLLdiscri = codeError, carrierFreq = carrFreq,
 * remPhase = remCarrPhase, and the remSample slot (that loop has no remSample) holds
 * absoluteSampleCodedelay. */
#define GNSS_F_carrError               GNSS_F_PLLdiscri
#define GNSS_F_codeError               GNSS_F_DLLdiscri
#define GNSS_F_carrFreq                GNSS_F_carrierFreq
#define GNSS_F_remCarrPhase            GNSS_F_remPhase
#define GNSS_F_absoluteSampleCodedelay GNSS_F_remSample

/* Outputs of trackingCT. Caller-allocated:
 *   rec      [nsv][GNSS_NFIELDS][max_len]  TckResultCT series per channel
 *            (series length 1000 + countinx + msToProcessCT_10ms, phase-C values
 *            written 10x as trackingCT.m:507-524 does); may be NULL.
 *   taps     [nsv][2][n_taps][max_len]     I then Q of every ACF tap; NULL unless
 *            wanted (phase-C taps are negated like E/P/L, trackingCT.m:447-449).
 *   len      [nsv]  series length per channel
 *   countinx [nsv]  bit-edge result (trackingCT.m:207)
 *   CN0_Eph  [cn0_cap][nsv] row-major (row = snrIndex-1); rows never written are 0
 *   cn0_rows  out: rows of the MATLAB CN0_Eph matrix
 *   flags     GNSS_OUT_DEVICE: rec and taps are DEVICE pointers (HIP memory of the
 *             ctx's device, e.g. gnss_dev_alloc or a framework tensor); the series are
 *             expanded into them on the GPU and never cross PCIe, so a multi-GPU caller
 *             can all-gather them over RCCL/xGMI as they lie. The call returns after the
 *             writes have completed (ctx stream synchronised). len, countinx and CN0_Eph
 *             stay host arrays. Not for gnss_tracking_ct_multicorr (its codedelay
 *             post-pass runs on the host): GNSS_EARG there.
 * max_len must be >= msToProcessCT_1ms + 19 + msToProcessCT_10ms.             */
#define GNSS_OUT_DEVICE 1
typedef struct gnss_track_out {
    int64_t  max_len;
    double  *rec;
    double  *taps;
    int64_t *len;
    int32_t *countinx;
    double  *CN0_Eph;
    int32_t  cn0_cap;
    int32_t  cn0_rows;
    int32_t  flags;     /* GNSS_OUT_DEVICE or 0 (ABI v7)                           */
    int32_t  reserved;
} gnss_track_out;

/* Device-side timing of the last call (hipEvents on the ctx stream). */
typedef struct gnss_timing {
    double acq_ms;            /* whole acquisition, IF resident in HBM             */
    double acq_corr_ms;       /* wipe + FFT correlation + power accumulation       */
    double acq_fine_ms;       /* fine-frequency FFTs + argmax                      */
    double track_ms;          /* whole trackingCT, IF resident in HBM              */
    double track_kernel_ms;   /* sum of correlator-kernel durations                */
    int64_t track_launches;   /* correlator-kernel launches                        */
    int64_t track_channel_samples;   /* channel-samples correlated (all taps)      */
    int64_t acq_hypothesis_samples;  /* PRN x bin x ms x Sample                     */
    double h2d_ms;            /* host->HBM upload of the IF window, if any         */
    /* profiling mode, the 10-ms phase (trackingCT.m:377-525) alone: the dominant
     * correlator kernel                                                           */
    double  track10_kernel_ms;
    int64_t track10_launches;
    int64_t track10_channel_samples;
    int64_t h2d_bytes;        /* bytes staged host/disk -> HBM in h2d_ms (ABI v8)  */
    int64_t track_segments;   /* 10-ms phase segments staged (gnss_ctx_set_window) */
} gnss_timing;

typedef struct gnss_ctx gnss_ctx;

int         gnss_abi_version(void);
const char *gnss_strerror(int status);

/* Create a context bound to HIP device `device` (owns stream, device buffers,
 * rocFFT plans). Replaces the MEX's persistent state (freed by mexAtExit). */
int  gnss_ctx_create(int device, gnss_ctx **out);
/* Multi-device context (ABI v11): one member context per entry of devices[0..n-1] (a device
 * may repeat; its members then run one after the other), so a MEX caller of SDR_main.m:22,38
 * shards over the GPUs of a node with no MATLAB change. gnss_acquisition deals the PRN list
 * (acquisition.m:47-80) and gnss_tracking_ct / _pos / _mc the channel list (trackingCT.m:22-528)
 * round-robin over the members, one host thread per device; each member keeps the global
 * svindex / nsv (quirk A.11), so every row is bit-identical to the one-context call. Results
 * are merged into the caller's arrays in the reference's order (Acquired and diag in PRN-list
 * order; tracking rows by channel). GNSS_OUT_DEVICE arrays live on devices[0]; a member on
 * another device expands its rows in its own HBM and copies them over xGMI (peer copies), and
 * a gnss_file.dev_data record on another device is copied range by range into each member's
 * HBM the same way. The status is the one-context call's (group.h). Every other entry point
 * runs on devices[0] alone. The setters apply to every member. n in 1..GNSS_MAX_DEVICES. */
#define GNSS_MAX_DEVICES 16
int  gnss_ctx_create_multi(const int *devices, int n, gnss_ctx **out);
/* Record residency of a multi-device context (ABI v12): a member on another device than a
 * gnss_file.dev_data record copies the WHOLE record into its own HBM by one peer copy (xGMI) the
 * first time a call reads it, and keeps that copy for every later call naming the same pointer
 * and length (gnss_timing.h2d_bytes counts the copy once). The library drops the copies that a
 * write of its own makes stale (gnss_dev_upload, gnss_synth_if_device into the record,
 * gnss_dev_free of it); a caller that rewrites the record by other means (its own hipMemcpy, a
 * MATLAB gpuArray) drops it here first. dev_ptr NULL drops every resident copy. The members'
 * copies are freed by gnss_ctx_destroy. No-ops for a one-device context. Replaces nothing in the
 * reference (SDR_main.m:22,38 re-read the file on every call). */
int  gnss_ctx_drop_record(gnss_ctx *ctx, const void *dev_ptr);
/* Resident record copies held by the context's members (0 for a one-device context). */
int  gnss_ctx_resident_records(const gnss_ctx *ctx);
/* HIP devices visible to this process (0 without a GPU or runtime). */
int  gnss_device_count(void);
/* Members of a context (1 for gnss_ctx_create). */
int  gnss_ctx_members(const gnss_ctx *ctx);
void gnss_ctx_destroy(gnss_ctx *ctx);
const char *gnss_last_error(const gnss_ctx *ctx);
int  gnss_last_timing(const gnss_ctx *ctx, gnss_timing *out);
/* Profiling mode: every correlator-step launch is bracketed by hipEvents (no
 * step graphs) so gnss_timing.track_kernel_ms is the sum of kernel durations. */
int  gnss_ctx_set_profiling(gnss_ctx *ctx, int enable);
/* Precision of the acquisition's PRN x bin x ms correlation (ABI v8; replaces nothing in
 * the reference, whose fft/ifft/abs().^2 are MATLAB doubles, acquisition.m:56-61):
 * fp64 = 1 (default) runs it at the reference's precision; fp64 = 0 is the fp32 fast mode
 * (the same decisions in every parity test, SNR within 1e-3 dB). The fine-frequency FFT
 * (acquisition.m:103-116) is fp64 in both. GNSS_EARG for other values. */
int  gnss_ctx_set_acq_precision(gnss_ctx *ctx, int fp64);
/* Streaming (ABI v8): at most `bytes` of IF resident in HBM per trackingCT call (0 = the
 * call's whole read range, the default). A record read from `path` or host `data` whose read
 * range exceeds it is staged in windows: the 1-ms phases' range first, then the 10-ms phase
 * (trackingCT.m:377-525) in segments of as many steps as the window holds, each staged through
 * the context's pinned double buffer before its launch (trackingCT.m:416-426 reads every step
 * from the file; the outputs are bit-identical to the unsegmented call). GNSS_EARG from the
 * call if the budget cannot hold the 1-ms phases' span or one 10-ms step of every channel. */
int  gnss_ctx_set_window(gnss_ctx *ctx, uint64_t bytes);
/* Test hooks (ABI v9; replace nothing in the reference): force one code path of the engine
 * so the parity tests can prove every path gives the reference's results. All default 0
 * (the engine's own choice); GNSS_EARG for an unknown key.                               */
#define GNSS_OPT_FORCE_SUB    0  /* lane span 8*v samples for both tracking phases (1..4) */
#define GNSS_OPT_NO_PERSIST   1  /* != 0: one launch per tracking step (no persistent loop;
                                    gnss_tracking_vt too, ABI v13)                        */
#define GNSS_OPT_FORCE_VPB    2  /* >= 2: virtual blocks per resident block of the loop     */
#define GNSS_OPT_ACQ_ROCFFT   3  /* != 0: rocFFT instead of the own P x 2000 correlator     */
#define GNSS_OPT_FINE_ROCFFT  4  /* != 0: rocFFT for the fine-frequency transform           */
#define GNSS_OPT_ACQ_BATCH    5  /* > 0: (bin, PRN) pairs per correlator batch (split path) */
#define GNSS_OPT_ACQ_FUSED    6  /* != 0: fp64 correlator as one persistent launch with the
                                    intermediate in each XCD's L2 (measured slower, kept
                                    for the record; default: two launches per batch)      */
#define GNSS_OPT_ACQ_RING     7  /* 2..4: ring slots per XCD of the fused correlator (3)    */
#define GNSS_OPT_ACQ_PIPE     8  /* split path: 1 = column and row passes of every batch in
                                    order on one stream, 2 = pipelined over two streams
                                    (batch b's rows beside batch b+1's columns, two
                                    intermediates), 3 = paired launches (fp64: batch
                                    b+1's column blocks and batch b's row blocks in one
                                    grid, interleaved; fp32 runs 2); 0 = the engine's
                                    choice                                                */
#define GNSS_OPT_VT_BLOCKS    9  /* 1..GNSS_VT_MAX_BLOCKS: blocks per channel of
                                    gnss_tracking_vt's step (GNSS_EARG above)             */
#define GNSS_OPT_FORCE_PEER   10 /* != 0 (multi-device contexts): every member treats
                                    dev_data and GNSS_OUT_DEVICE arrays as on another
                                    device (range copies in, row copies out), so one GPU
                                    exercises the peer-copy path                          */
#define GNSS_OPT_VT_SPAN      11 /* 1..2000 (ABI v13): steps per staged IF window of
                                    gnss_tracking_vt on a host record (2000; GNSS_EARG
                                    outside), so a short loop exercises the re-staging   */
#define GNSS_OPT_SLOT_PATH    12 /* the <= 3-tap correlators' tap prefixes, for tests and A/B:
                                    1 = through the LDS running-sum slots (as above 3
                                    taps) everywhere, 2 = from the capture register
                                    everywhere (a lane with a second boundary then takes
                                    the rolled second pass); 0 = by gnss_lane_boundaries  */
#define GNSS_OPT_COUNT        13
int  gnss_ctx_set_option(gnss_ctx *ctx, int key, int64_t value);
/* The most distinct chip-boundary samples one correlator lane of `lane_samples` samples can hold
 * for a tap set (`post` may be NULL) while the code advances at most `cps_max` chips per
 * sample: taps a whole number of chips apart share their boundary and count once, plus one
 * sample for rounding (one more per further set of two or more taps). The <= 3-tap correlators
 * keep their tap prefixes in registers where this is at most 2, i.e. one boundary set per lane
 * (E/P/L at 58 MHz, lanes up to 24 samples), else in the LDS slots. -1 for bad arguments.    */
int  gnss_lane_boundaries(const double *taps, const double *post, int n_taps, int lane_samples,
                          double cps_max);
/* 1 when the context's last gnss_tracking / gnss_correlate_step ran the register-capture
 * correlator for every lane span it used, 0 when any ran through the LDS slots. The choice is
 * made when the call is planned: the value is meaningful on a single-device context after a
 * call that returned GNSS_OK (a multi-device context's members plan their own calls; the
 * group's value stays 0).                                                                   */
int  gnss_ctx_lane_path(const gnss_ctx *ctx);

/* Device memory owned by the ctx, for callers that keep an IF record resident
 * in HBM (gnss_file.dev_data) across calls. */
int  gnss_dev_alloc(gnss_ctx *ctx, uint64_t nbytes, void **dev_ptr);
int  gnss_dev_free(gnss_ctx *ctx, void *dev_ptr);
int  gnss_dev_upload(gnss_ctx *ctx, void *dev_dst, const void *host_src, uint64_t nbytes);
int  gnss_dev_download(gnss_ctx *ctx, void *host_dst, const void *dev_src, uint64_t nbytes);

/* acquisition.m replacement (acquisition.m:1-127). Returns GNSS_ENODATA with
 * out->n == 0 when nothing is acquired (acquisition.m:84-85). diag may be NULL. */
int gnss_acquisition(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                     const gnss_acq *acq, gnss_acquired *out, gnss_acq_diag *diag);

/* trackingCT.m replacement (trackingCT.m:1-530). The `countinx.mat` side file
 * (trackingCT.m:530) is the wrapper's job (MEX / Python mirror).
 * Sampling-rate floor (this call, its _pos / _mc / _multicorr variants and
 * gnss_correlate_step): the correlator's lanes take 8 samples at least and hold at most one
 * chip boundary per tap, so Fs must exceed 8 * 1.01 * codeFreqBasis (8.26584 MHz for the
 * C/A code; gnss_correlate_step also 8 * its codeFreq argument). A lower rate is refused on
 * the host, before any launch, with GNSS_EARG and a gnss_last_error text naming the floor
 * (MATLAB runs such a rate, so it is no GNSS_EINDEX); the context stays usable. Every rate
 * above the floor runs: no admitted rate ends in GNSS_EINDEX for its lane geometry. */
int gnss_tracking_ct(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                     const gnss_track *track, const gnss_acquired *acquired,
                     gnss_track_out *out);

/* The tracking loop of trackingCT_POS_updated.m (its positioning half,
 * :420-565, is gnss_ct_pos_solve, a pass over this call's records). Replaces the per-channel correlator / NCO / DLL / PLL of
 * trackingCT_POS_updated.m:92-144,179-413:
 *   - file_ptr = (Sample - codedelay + 1 + skip*Sample)*bytes (:108-110), one continuous
 *     read per channel (no re-seek at the 1 -> 10 ms switch);
 *   - steps msIndex = 1..ctPOS (track.ctPOS, :50); pdi = 1 while msIndex <= 1000 +
 *     countinx[svIndex] (:183; 1000 = track.msToProcessCT_1ms, countinx as loaded from
 *     countinx.mat at :29, indexed by channel POSITION), else 10;
 *   - numSample = ceil(...) (:189); E/P/L at Spacing(3) = +0.5, prompt Code(ceil(t+0.05)+1),
 *     Spacing(23) = -0.5 (:42,210-217); no negation; codeFreq = f0 + codeNco (:262);
 *     loop filters with T = signal.ms at every pdi (:257,266);
 *   - C/N0 every 20 steps of either pdi into one CN0_CT (:237-250);
 *   - one record row per step (Index = msIndex), codedelay = Sample - codedelay + 1 +
 *     sum(delayValue(svIndex,1:Index)) (:290).
 * out: rec[nsv][GNSS_NFIELDS][max_len] (max_len >= ctPOS, len = ctPOS), CN0_Eph = CN0_CT
 * (cn0_rows = ctPOS/20), countinx echoed. int8 records only (GNSS_EARG for int16: the
 * reference advances file_ptr by numSample*dataType bytes after reading twice that,
 * :196,207). EOF inside the loop -> GNSS_EIO (MATLAB raises on the short vector).    */
int gnss_tracking_ct_pos(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                         const gnss_track *track, const gnss_acquired *acquired, int32_t ctPOS,
                         const int32_t *countinx, gnss_track_out *out);

/* The tracking loop of trackingCT_POS_updated_multicorrelator.m (the
 * 25-tap sibling; its positioning half, :446-590, is gnss_ct_pos_solve with
 * GNSS_CT_POS_MULTICORR on this call's records). Replaces the channel
 * loop of trackingCT_POS_updated_multicorrelator.m:41-136,170-440:
 *   - steps msIndex = 1..msPosCT/pdi (datalength = track.msPosCT, pdi = track.pdi, :46-49,
 *     :170; pdi 1 or 10), every step at that pdi, one continuous read per channel from
 *     file_ptr = (Sample - codedelay + 1 + skip*Sample)*bytes (:101-103);
 *   - GNSS_MC_TAPS taps at Spacing = 0.6:-0.05:-0.6 (:41), replica Code(ceil(t) + 2) with
 *     Code = [CA(end) repmat(CA,1,pdi) CA(1) CA(2)] (:94,233-258), no +0.05 on the prompt;
 *     E/P/L = Spacing(3)/(13)/(23) feed the DLL/PLL; numSample = ceil(...) (:177);
 *     codeFreq = f0 + codeNco; loop filters with T = pdi*t (:351-364);
 *   - C/N0 every 20 steps with 1/(t*pdi) (:333-345);
 *   - one record row per step (the fields of :428-439 in gnss_track_out.rec as for
 *     gnss_tracking_ct_pos), every tap in gnss_track_out.taps[nsv][2][25][max_len] in
 *     Spacing order (E_i_060 ... L_i060 of :374-423).
 * max_len >= msPosCT/pdi; track->n_taps must be 0. int8 records only, EOF -> GNSS_EIO. */
#define GNSS_MC_TAPS 25

/* trackingCT_multiCorr-GIVEN.m (function trackingCT_multiCorr, the multi-correlator loop the
 * assignment hands out). Replaces TckResultCT = trackingCT_multiCorr(file,
 * signal, track, Acquired) (:1): per channel, fseek to (Sample - codedelay - 1 + skip*Sample)
 * bytes*2 (:57) and `datalength` 1-ms steps (:27 hard-codes 50000) read continuously, with
 * trackingCT.m's loop (round -> ceil for numSample, :60; remChip from codeFreqBasis*ms;
 * codeFreq = f0 - code_output; T = 1 ms) on the GNSS_MC_TAPS taps Spacing = -0.6:0.05:0.6
 * (:25), Code(ceil(t) + 1), E/P/L = Spacing(3)/(13)/(23) = -0.5/0/+0.5. Records as
 * gnss_tracking_ct (rec fields of :287-297 in the trackingCT slots, remSample included; every
 * tap in taps[nsv][2][25][max_len], the E_i_060 ... L_q060 of :163-286), one row per step;
 * codedelay = codedelay + sum(delayValue(1:msIndex)) over ONE nsv x datalength matrix filled
 * channel after channel (:29,297: earlier channels' rows count whole). CN0_CT every 20 steps.
 * max_len >= datalength; int8 I/Q records only (:47-48 pairs every record), no channel shard;
 * a short read -> GNSS_EIO (MATLAB raises; the function has no "Not enough raw data" branch). */
int gnss_tracking_ct_multicorr(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                               const gnss_track *track, const gnss_acquired *acquired,
                               int32_t datalength, gnss_track_out *out);
int gnss_tracking_ct_mc(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                        const gnss_track *track, const gnss_acquired *acquired, int32_t msPosCT,
                        int32_t pdi, gnss_track_out *out);

/* ---- naviDecode_updated.m ---------------------------------
 * Navigation-bit decode on the tracking output: bit synchronisation of P_i, preamble
 * search, parity (paritychk_James.m) and subframe 1-3 fields (bin2dec_GPSSDR.m,
 * comp2dec.m), with the reference's behaviour kept (repeat decodes are appended; bit
 * arrays carry over between channels — see csrc/navdecode.cpp).
 * Replaces [ephemeris, ~, for_prest] = naviDecode_updated(Acquired, ALLTckResult)
 * (naviDecode_updated.m:1, called at SDR_main.m:54). Channel c's ephemeris(prn) is
 * eph[c][field][0 .. eph_len[c][field]), prn = acquired->sv[c]. Host code (no GPU). */
enum gnss_eph_field {
    GNSS_E_TOW = 0, GNSS_E_TOW1, GNSS_E_sfb, GNSS_E_sfb1, GNSS_E_weeknum, GNSS_E_N, GNSS_E_health,
    GNSS_E_IODC, GNSS_E_TGD, GNSS_E_toc, GNSS_E_af2, GNSS_E_af1, GNSS_E_af0, GNSS_E_IODE2, GNSS_E_Crs,
    GNSS_E_deltan, GNSS_E_M0, GNSS_E_Cuc, GNSS_E_ecc, GNSS_E_Cus, GNSS_E_sqrta, GNSS_E_toe, GNSS_E_Cic,
    GNSS_E_omegae, GNSS_E_Cis, GNSS_E_i0, GNSS_E_Crc, GNSS_E_w, GNSS_E_omegadot, GNSS_E_IODE3,
    GNSS_E_idot, GNSS_E_updatetime, GNSS_E_updatetime_tow,
    GNSS_EPH_NFIELDS
};

typedef struct gnss_nav_out {
    int32_t  eph_cap;     /* values per field per channel (GNSS_EARG if one overflows) */
    double  *eph;         /* [nsv][GNSS_EPH_NFIELDS][eph_cap]                            */
    int32_t *eph_len;     /* [nsv][GNSS_EPH_NFIELDS]                                     */
    int32_t *updateflag;  /* [nsv] ephemeris(prn).updateflag                             */
    int64_t *nav1;        /* [nsv] for_prest.nav1(prn): first P_i index of the bit stream */
    int64_t *sfb1;        /* [nsv] for_prest.sfb1(prn): first subframe 1 (0 if none)      */
} gnss_nav_out;

/* P_i of channel c at P_i[c*stride + k], k < len[c] (TckResultCT(sv[c]).P_i). */
int gnss_navi_decode(const gnss_acquired *acquired, const double *P_i, const int64_t *len,
                     int64_t stride, gnss_nav_out *out);

/* Per-step parity hook: ONE trackingCT correlation step (trackingCT.m:79-118: numSample
 * from remChip/codeFreq, E/P/L or ACF replicas, carrier wipe, sums; no negation, no
 * loop update) at an arbitrary NCO state, on the same kernel the tracker launches.
 * sums_out[2*n_taps] = (I, Q) per tap; taps as gnss_track.tap_offsets (3 or 11). */
int gnss_correlate_step(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                        int prn, int pdi, double remChip, double codeFreq, double carrierFreq,
                        double remPhase, int64_t pos_bytes, int n_taps, const double *taps,
                        double *sums_out, int64_t *numSample_out);

/* Parity hook (ABI v14): the acquisition's whole correlation surface, for tests that compare
 * every cell with an independent evaluation of acquisition.m:41-61. Runs gnss_acquisition's
 * own coarse half (the same staging, the same correlator under the context's precision and
 * GNSS_OPT_ACQ_* options, the same detector), then copies the surface back:
 *   surface_out[(p * freqNum + b) * Sample + tau], p over the PRN list, b the Doppler bin, tau
 *   the code-phase column in natural order (the own correlator's tau2-major storage is undone
 *   on the host); an fp32 surface (gnss_ctx_set_acq_precision(ctx, 0)) is widened to double.
 * diag (may be NULL) is filled as gnss_acquisition fills it, from that same surface. No fine
 * search runs, and GNSS_OK is returned also when no PRN clears the 12 dB gate. Single-device
 * contexts only (GNSS_EARG on a multi-device one). Not a product path: the surface crosses
 * PCIe and is reordered by the host.                                                        */
int gnss_acquisition_surface(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                             const gnss_acq *acq, double *surface_out, gnss_acq_diag *diag);

/* ---- trackingVT_POS_updated.m, the tracking half (ABI v9) -----------
 * Steps of the loop at trackingVT_POS_updated.m:157-349 for n channels: read sizing (:161),
 * the three replica chips, the carrier wipe and sums (:217-281), the remaining code /
 * carrier phase (:284-285), the C/N0 estimator (:292-304), the PLL (:305-311) and the DLL
 * discriminator (:314-316). The vector half -- satellite position, iono / tropo, the
 * predicted code frequency and the Kalman filter (:166-215, :350-420) -- stays with the
 * caller, which passes each step's predicted code frequency.
 * The reference's replica quirk is kept: Code(svindex, ceil_mx(1)) linear-indexes ONE
 * element of the 3 x n matrix ceil_mx (the first sample's chip of each of the E / P / L
 * rows, the 1025 clamp of :240-246 applied to it alone), so E / P / L = that chip times
 * the whole sum(InphaseSignal) / sum(QuadratureSignal). Spacing = 0.7:-0.05:-0.7 (:27):
 * E / P / L at Spacing(5) / (15) / (25) = +0.5 / 0 / -0.5; the three colons must have
 * numSample elements each (ceil_mx's vertical concatenation and t_CodePrompt(numSample),
 * :217-228, :284), else GNSS_EINDEX as MATLAB raises.
 * Formats (:163-176): int8 I/Q (dataPrecision 1, dataType 2), int8 real (1, 1), int16 I/Q
 * with each read's means removed (2, 2); file_ptr in bytes. */
typedef struct gnss_vt_chan {
    int32_t prn;
    int32_t pad;
    int64_t file_ptr;       /* bytes: the fseek position of the next read (:162)          */
    double  remChip;        /* chips (:284)                                               */
    double  remCarrPhase;   /* rad (:285)                                                 */
    double  codeFreq;       /* the last step's code frequency: sizes the next read (:161) */
    double  carrFreq;       /* carrier NCO frequency (:310)                               */
    double  carrFreqBasis;  /* (:121)                                                     */
    double  oldCarrNco, oldCarrError;  /* PLL filter state (:307-308)                    */
    int32_t index_int;      /* C/N0 estimator (:78-81, :293-303): Zk entries filled, 0..19 */
    int32_t snrIndex;       /*   the next CN0_VT row (1-based; starts at 1)                */
    double  Zk[20];         /*   P_i^2 + P_q^2 of the current K = 20 block                 */
} gnss_vt_chan;

/* TckResultVT(prn).*(msIndex) of one channel and step (:319-346) and CN0_VT. */
typedef struct gnss_vt_out {
    double  E_i, E_q, P_i, P_q, L_i, L_q;
    double  carrError, codeError, carrNco;
    double  remChip, remCarrPhase, codeFreq, carrFreq;
    int64_t numSample, absoluteSample;
    double  codedelay;
    double  CN0;            /* CN0_VT(cn0_row, svindex) when cn0_row > 0 (:301)           */
    int32_t cn0_row;        /* 1-based row written by this step, 0: none                  */
    int32_t status;         /* GNSS_OK, or the channel's error at this step (vt_run)      */
    /* ABI v10, written by gnss_tracking_vt (the vector half; 0 from vt_run / vt_step):     */
    double  deltaPr;        /* TckResultVT(prn).deltaPr(msIndex) (:221,351), m/s          */
    double  prRate;         /* TckResultVT(prn).prRate: never assigned in the loop, 0 (:142) */
    double  sv_vel[3];      /* TckResultVT(prn).sv_vel(msIndex,:) (:185,346), m/s ECEF     */
} gnss_vt_out;

/* nsteps steps of the n channels in ONE launch (one workgroup per channel loops over the
 * steps: read sizing, sums in a fixed order, the scalar end, all on the GPU):
 * codeFreq_new[s * n + i] = channel i's code frequency for step s (:211-215; the caller's
 * EKF prediction, or a recorded series), pdi = track.pdi. chans[] are advanced in place;
 * out[s * n + i] = channel i's record of step s. A channel whose step fails (GNSS_EINDEX: a
 * replica index MATLAB would reject; GNSS_EIO: read past EOF) stops there with
 * out[..].status set; the call returns the first such status. */
int gnss_tracking_vt_run(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                         const gnss_track *track, int32_t pdi, int32_t n, int32_t nsteps,
                         gnss_vt_chan *chans, const double *codeFreq_new, gnss_vt_out *out);

/* One step: gnss_tracking_vt_run with nsteps = 1. */
int gnss_tracking_vt_step(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                          const gnss_track *track, int32_t pdi, int32_t n, gnss_vt_chan *chans,
                          const double *codeFreq_new, gnss_vt_out *out);

/* The same step's host half alone (no GPU): from the channel state, this step's code
 * frequency and the step's carrier-wiped sums (sumI = sum(InphaseSignal), sumQ =
 * sum(QuadratureSignal)), the record and the advanced state -- the arithmetic the
 * kernel's scalar end runs (the same source). int8 I/Q byte offsets. */
int gnss_vt_nco_step(const gnss_signal *signal, const gnss_track *track, int32_t pdi,
                     gnss_vt_chan *chan, double codeFreq_new, double sumI, double sumQ,
                     gnss_vt_out *out);

/* The replica chips and read size of a VT step (host, no GPU): code[3] = the E / P / L
 * chip values (+-1) the quirk multiplies the sums by, *numSample = ceil(...) (:161). */
int gnss_vt_prepare(const gnss_signal *signal, int32_t pdi, const gnss_vt_chan *chan,
                    double codeFreq_new, int32_t code_out[3], int64_t *numSample);

/* ---- trackingVT_POS_updated.m, the vector half (ABI v10) -------------
 * The EKF that drives the VT loop's code NCOs: per step and channel, the satellite position
 * at the block's transmit time (svPosVel.m), the iono / tropo corrections every 0.1 s
 * (ionocorr.m, trop_UNB3.m), the predicted pseudorange with the earth-rotation correction
 * (erotcorr.m) and from it the code frequency (:180-227); after the step's correlations the
 * 8-state EKF (position, velocity, clock bias, clock drift) on the 2n code and carrier
 * measurements (:357-442) and the adaptive measurement noise (:444-467). Host C++ (fp64 with
 * MATLAB's operation order, -ffp-contract=off); libm's sin / cos / atan2 / pow and MATLAB's
 * BLAS-backed matrix products and inv() round differently in the last place, so the values
 * match the reference within the ulp bounds stated in tests/test_vt_nav_kat.py. */
#define GNSS_VT_MAX_CH 32
#define GNSS_VT_MAX_BLOCKS 1024  /* blocks per channel of one VT step (GNSS_OPT_VT_BLOCKS)  */

/* ephemeris(prn).*(eph_idx) -- the fields svPosVel.m:23-44 reads (eph_idx = 1, :36). */
typedef struct gnss_eph_sv {
    double sqrta, deltan, toe, M0, ecc, w, Cus, Cuc, Crs, Crc, Cis, Cic, i0, idot, omegae, omegadot;
    double toc, af0, af1, af2, TGD;
} gnss_eph_sv;

/* The inputs of the vector half beyond the tracking structs: cnslxyz, the iono model
 * (initParameters.m:29-31), cmn.doy / cmn.cSpeed, signal.Fc. */
typedef struct gnss_vt_nav_cfg {
    double cnslxyz[3]; /* the cnslxyz argument (SDR_main.m:66: llh2xyz(solu.iniPos)), ECEF m:
                          the ionocorr user position (:200) and the navSolutionsVT ENU
                          origin (:407-415)                                                  */
    double ALPHA[4];   /* global ALPHA, BETA: broadcast iono model (initParameters.m:29-30)  */
    double BETA[4];
    double doy;        /* cmn.doy (trop_UNB3, :201)                                          */
    double cSpeed;     /* cmn.cSpeed, m/s                                                    */
    double Fc;         /* signal.Fc, Hz (the carrier's pseudorange rate, :380)               */
} gnss_vt_nav_cfg;

/* The loop's navigation state (all of trackingVT_POS_updated.m's cross-step variables other
 * than the channels' NCO state, which is gnss_vt_chan). Caller-allocated POD: init fills it,
 * predict / update advance it; it may be copied (a checkpoint) between steps. */
typedef struct gnss_vt_nav {
    int32_t n, pdi;
    int32_t msIndex;            /* the step being run: 1-based, advanced by update        */
    int32_t counterUptR, counter_r;
    int32_t prn[GNSS_VT_MAX_CH];
    gnss_vt_nav_cfg cfg;
    double  Fs, IF, codeFreqBasis, ms;
    double  cnslxyz[3];
    double  total_state[8];     /* [estPos estVel clkBias clkDrift] (:70, :400, :440)     */
    double  state_cov[64];      /* row-major 8 x 8 (:49, :391, :398)                      */
    double  R[2 * GNSS_VT_MAX_CH];     /* diag(mesurement_noise) (:55-56, :447-462)      */
    double  recordR2[2 * GNSS_VT_MAX_CH]; /* sum(recordR.^2) over the rows since the last
                                             noise update (:395, :446)                    */
    double  transmitTime[GNSS_VT_MAX_CH];  /* transmitTimeVT (:131, :181)                 */
    double  tot_est_tck[GNSS_VT_MAX_CH];   /* this step's (:182)                          */
    double  predictedPr_last[GNSS_VT_MAX_CH];
    double  counter_corr[GNSS_VT_MAX_CH];  /* (:86, :189-204)                             */
    double  ionodel[GNSS_VT_MAX_CH], tropodel[GNSS_VT_MAX_CH];
    double  el[GNSS_VT_MAX_CH], az[GNSS_VT_MAX_CH];   /* degrees (:195-196)               */
    int64_t numSample[GNSS_VT_MAX_CH];     /* this step's reads (:164)                    */
    gnss_eph_sv eph[GNSS_VT_MAX_CH];
} gnss_vt_nav;

/* navSolutionsVT.*(msIndex,:) of one step (:418-436). The 2n-long rows hold the code
 * measurements (channels 0..n-1) then the carrier ones (n..2n-1). */
typedef struct gnss_vt_navsol {
    double localTime;
    double usrPos[3], usrVel[3];
    double usrPosENU[3], usrVelENU[3], usrPosLLH[3];   /* LLH: degrees, degrees, m       */
    double clkBias, clkDrift;
    double state[8];              /* error_state after the update (:428)                  */
    double state_cov[8];          /* diag(state_cov) (:431)                               */
    double newZ[2 * GNSS_VT_MAX_CH];
    double meas_inno[2 * GNSS_VT_MAX_CH];
    double satEA[GNSS_VT_MAX_CH], satAZ[GNSS_VT_MAX_CH];  /* el / az, degrees             */
    double predicted_z[2 * GNSS_VT_MAX_CH];  /* H_pos * error_state (:434)               */
    double satePos[3], sateVel[3]; /* svxyzr_pos / sv_vel_pos of the LAST channel (:426-427:
                                      svindex is the loop's last value there)             */
    double svxyz_pos[GNSS_VT_MAX_CH][3];  /* navSolutionsVT.svxyz_pos(:,:,msIndex) (:429)  */
    double kalman_gain[8][2 * GNSS_VT_MAX_CH]; /* (:430), columns 0..2n-1 used           */
    double R[2 * GNSS_VT_MAX_CH]; /* navSolutionsVT.R(counter_r,:) when r_row > 0 (:466) */
    int32_t r_row;                /* 1-based row of navSolutionsVT.R written, 0: none     */
    int32_t reserved;
} gnss_vt_navsol;

/* svPosVel.m: SV position / velocity (ECEF), clock correction (m, m/s) and group delay (s)
 * at transmit time t (GPS seconds of week). Any output pointer may be NULL. */
int gnss_sv_pos_vel(const gnss_eph_sv *eph, double t, double pos[3], double vel[3],
                    double *clkcorr_m, double *clkcorr_m_vel, double *grpdel);
/* The SDR_MATLAB-main/geo helpers the loop uses, exported for their known-answer tests:
 *   GNSS_GEO_XYZ2LLH  in xyz[3]            -> out llh[3] (rad, rad, m)   xyz2llh.m
 *   GNSS_GEO_LLH2XYZ  in llh[3]            -> out xyz[3]                 llh2xyz.m
 *   GNSS_GEO_XYZ2ENU  in xyz[3], org[3]    -> out enu[3]                 xyz2enu.m
 *   GNSS_GEO_EROTCORR in svxyz[3], pr      -> out svxyzr[3]              erotcorr.m
 *   GNSS_GEO_IONO     in t, svxyz[3], usrxyz[3], ALPHA[4], BETA[4] -> out[0] m  ionocorr.m
 *   GNSS_GEO_TROP     in doy, lat (deg), alt (m), el (deg)   -> out[0] m  trop_UNB3.m  */
#define GNSS_GEO_XYZ2LLH  0
#define GNSS_GEO_LLH2XYZ  1
#define GNSS_GEO_XYZ2ENU  2
#define GNSS_GEO_EROTCORR 3
#define GNSS_GEO_IONO     4
#define GNSS_GEO_TROP     5
int gnss_geo(int fn, const double *in, double *out);

/* The loop's initialisation (:39-86, :109-155): the EKF (Transistion_Matrix with pdi * ms,
 * state_cov, process / measurement noise), total_state from the navigation solution of the
 * scalar loop at row skiptimeVT/navSolPeriod (usrPos, usrVel, clkBias, clkDrift, :66-70),
 * transmitTimeVT = navSolutionsCT.timeTransmit(1, :) (:131), counters. prn[n], eph[n] per
 * channel in Acquired.sv order. The channels' NCO state (gnss_vt_chan) comes from
 * TckResultCT at msStartTckVT (:114-124); the caller builds it (sdr.trackingVT_POS_updated).
 * pdi = track.pdi. GNSS_EARG for n outside 1..GNSS_VT_MAX_CH. */
int gnss_vt_nav_init(const gnss_vt_nav_cfg *cfg, const gnss_signal *signal, int32_t pdi, int32_t n,
                     const int32_t *prn, const gnss_eph_sv *eph, const double usrPos[3],
                     const double usrVel[3], double clkBias, double clkDrift,
                     const double *timeTransmit, gnss_vt_nav *nav);

/* The tracking-side prediction for channel i of step nav->msIndex (:180-227): advance the
 * transmit time by numSample / Fs (the step's read, sized with the LAST code frequency, :164),
 * svPosVel at it, the iono / tropo update every corrUpt steps, the predicted pseudorange
 * and, from step 2 on, codeFreq = codeFreqBasis * (1 - deltaPr / c); at step 1 *codeFreq is
 * left as passed (TckResultCT's codeFreq(msStartTckVT), :218-219). Outputs the step's
 * deltaPr and sv_vel. */
int gnss_vt_nav_predict(gnss_vt_nav *nav, int32_t i, int64_t numSample, double *codeFreq,
                        double *deltaPr, double sv_vel[3]);

/* The navigation update after every channel's correlation of step nav->msIndex (:357-467):
 * measurements Z = [codeError * c / codeFreq ; prr_predicted - prr_measured - clkDrift +
 * sv_clk_vel] from each channel's codeError, codeFreq and carrFreq (TckResultVT of this
 * step), the Kalman update, the state prediction for the next step and, every
 * 200 / pdi steps, the measurement-noise update. sol (may be NULL) receives the
 * navSolutionsVT row. Advances nav->msIndex. */
int gnss_vt_nav_update(gnss_vt_nav *nav, const double *codeError, const double *codeFreq,
                       const double *carrFreq, gnss_vt_navsol *sol);

/* The whole loop (trackingVT_POS_updated.m:157-476) for nsteps = msToProcessVT / pdi steps:
 * per step, every channel's read size and predicted code frequency on the host, the
 * correlations and NCO / PLL / DLL / C/N0 of all channels in one launch of the VT kernel
 * (vt.hip; chans stay resident in HBM), then the EKF on the host. chans[n] and *nav advance
 * in place; out[s * n + i] = TckResultVT(Acquired.sv(i)).*(s + 1) incl. deltaPr / prRate /
 * sv_vel; sol[s] (may be NULL) = navSolutionsVT row s + 1. A channel error (a replica index
 * MATLAB rejects, a read past EOF) stops the loop at that step (MATLAB raises): the step's
 * records hold the status, the call returns it. */
int gnss_tracking_vt(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                     const gnss_track *track, int32_t n, int32_t nsteps, gnss_vt_chan *chans,
                     gnss_vt_nav *nav, gnss_vt_out *out, gnss_vt_navsol *sol);

/* ---- trackingVT_POS_updated_multicorrelator.m: the 25-tap vector-tracking loop ------------
 * Additive within ABI v13: new symbols and one new struct, no existing layout or meaning
 * changes and gnss_abi_version() stayed 13; a caller detects these entry points by symbol
 * (dlsym / hasattr). Line cites below are of trackingVT_POS_updated_multicorrelator.m.
 *
 * The loop SDR_main.m runs for cmn.mltCorrON = [1 1]. It is trackingVT_POS_updated.m except:
 * Spacing = 0.6:-0.05:-0.6 (:26), 25 taps, E / P / L = Spacing(3) / (13) / (23) = +0.5 / 0 /
 * -0.5; every sample of every tap is despread against a real replica Code(ceil(t) + 2) of
 * Code = [c(end) c(end-1) repmat(c,1,pdi) c(1) c(2)] (:104, :230-281; the pad's order is the
 * reference's: ceil(t) = 0 reads c(end-1), -1 reads c(end)), so E / P / L are real sums and
 * codeError a real early-late discriminator; remChip comes from the prompt colon (:354); the
 * EKF measures prr with carrFreq - signal.IF (:504); and there is no msStartTckVT clamp.
 * GNSS_EINDEX where MATLAB raises: a tap colon without exactly numSample elements, or a table
 * index outside 1 .. 1023 * pdi + 4. Formats as gnss_tracking_vt_run. */
#define GNSS_VT_MC_TAPS 25

/* TckResultVT_mltCorr(prn).*(msIndex): gnss_vt_out's fields, then the 50 tap sums in Spacing
 * order (E_i_060 .. E_i_005, P_i, L_i005 .. L_i060 and the _q twins, :401-450). E_i / P_i /
 * L_i (and _q) equal taps 2 / 12 / 22. */
typedef struct gnss_vt_mc_out {
    double  E_i, E_q, P_i, P_q, L_i, L_q;
    double  carrError, codeError, carrNco;
    double  remChip, remCarrPhase, codeFreq, carrFreq;
    int64_t numSample, absoluteSample;
    double  codedelay;
    double  CN0;
    int32_t cn0_row;
    int32_t status;
    double  deltaPr;        /* written by gnss_tracking_vt_mc (0 from gnss_tracking_vt_mc_run) */
    double  prRate;
    double  sv_vel[3];
    double  tap_i[GNSS_VT_MC_TAPS];
    double  tap_q[GNSS_VT_MC_TAPS];
} gnss_vt_mc_out;

/* The tracking half (:151-470) with the caller's code frequency per step, one launch of the
 * 25-tap correlator per step (csrc/vt_mc.hip): codeFreq_new[s * n + i], chans[] and out[s * n +
 * i] as gnss_tracking_vt_run, n in 1..GNSS_VT_MAX_CH. The host sizes every read and clears it
 * against the record before the launch: a channel whose step fails (GNSS_EINDEX; GNSS_EIO: read
 * past EOF) stops there with out[..].status set and sits the later steps out (zero records);
 * the call returns the first such status. GNSS_OPT_VT_BLOCKS sets the blocks per channel,
 * GNSS_OPT_VT_SPAN the steps per staged IF window. */
int gnss_tracking_vt_mc_run(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                            const gnss_track *track, int32_t pdi, int32_t n, int32_t nsteps,
                            gnss_vt_chan *chans, const double *codeFreq_new, gnss_vt_mc_out *out);

/* The whole loop (:151-609) with the EKF: nav as initialised by gnss_vt_nav_init, each step's
 * code frequency from gnss_vt_nav_predict, the update with prr_measured = (carrFreq - IF) * c /
 * Fc. Arguments and the stop at a channel error as gnss_tracking_vt. */
int gnss_tracking_vt_mc(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                        const gnss_track *track, int32_t n, int32_t nsteps, gnss_vt_chan *chans,
                        gnss_vt_nav *nav, gnss_vt_mc_out *out, gnss_vt_navsol *sol);

/* The step's host half alone (no GPU). Prepare: *numSample = ceil(...) (:155) and each tap's
 * colon ends -- element k of tap j is MATLAB's colon element of {tap_a[j], codeFreq_new / Fs,
 * tap_c[j]} with numSample elements (tap_a / tap_c / numSample may be NULL) -- or GNSS_EINDEX. */
int gnss_vt_mc_prepare(const gnss_signal *signal, int32_t pdi, const gnss_vt_chan *chan,
                       double codeFreq_new, double tap_a[GNSS_VT_MC_TAPS],
                       double tap_c[GNSS_VT_MC_TAPS], int64_t *numSample);

/* ... and the scalar end (:354-391) from the step's 50 sums in Spacing order: the record and
 * the advanced channel state. int8 I/Q byte offsets. */
int gnss_vt_mc_nco_step(const gnss_signal *signal, const gnss_track *track, int32_t pdi,
                        gnss_vt_chan *chan, double codeFreq_new,
                        const double tap_i[GNSS_VT_MC_TAPS], const double tap_q[GNSS_VT_MC_TAPS],
                        gnss_vt_mc_out *out);

/* gnss_vt_nav_update with the 25-tap loop's measurement prr_measured = (carrFreq - IF) * c / Fc
 * (:504); everything else is gnss_vt_nav_update's. */
int gnss_vt_mc_nav_update(gnss_vt_nav *nav, const double *codeError, const double *codeFreq,
                          const double *carrFreq, gnss_vt_navsol *sol);

/* ---- trackingCT_POS_updated.m, the positioning half: navSolutionsCT ---------------------------
 * Additive within ABI v13, like the 25-tap loop above: one status, two structs and one entry
 * point, no existing layout or meaning changes and gnss_abi_version() stayed 13; a caller detects
 * the entry point by symbol. Line cites are of trackingCT_POS_updated.m unless marked.
 *
 * Positioning does not feed back into the scalar loops, so it runs as a pass over the records of
 * gnss_tracking_ct_pos / gnss_tracking_ct_mc (:147-171, :420-565, with olspos.m, hmat.m and
 * LS_SA_code_Vel.m; fp64 in the reference's association order, -ffp-contract=off):
 *   - sampleStartMea = max(sampleStart) + 1 (:160), measSampleStep = fix(Fs * navSolPeriod / 1000)
 *     * dataType (:164), currMeasSample = sampleStartMea + measSampleStep * posIndex (:423);
 *   - at tracking step Index an epoch fires iff every channel's absoluteSample(Index) >
 *     currMeasSample (:427-435): at most one epoch per step, so with navSolPeriod shorter than the
 *     step the solution lags and does not catch up;
 *   - per channel, index = (first i with absoluteSample(i) > currMeasSample) - 1 (:442-447;
 *     index = 0 -> GNSS_EINDEX, MATLAB raises at :450) and codePhaseMeas = remChip(index) +
 *     (codeFreq(index) / Fs) * ((currMeasSample - absoluteSample(index)) / dataType) (:450-453);
 *   - transmitTime (:455-457), GNSS_CT_POS_UPDATED: codePhaseMeas / codelength / 1000 + ((index -
 *     ms1 - countinx(s)) * pdi + (ms1 + countinx(s)) - (nav1 + sfb1 * 20)) / 1000 + TOW1 with pdi
 *     the loop variable as the LAST channel's branch left it at step Index (1 if Index <= ms1 +
 *     countinx(n), else 10; :183-184,294-295) and ms1 = msToProcessCT_1ms; GNSS_CT_POS_MULTICORR
 *     (trackingCT_POS_updated_multicorrelator.m:481-483): codePhaseMeas / codelength / 1000 +
 *     (index - (nav1 + sfb1 * 20)) / 1000 + TOW1 whatever pdi is;
 *   - first fix: localTime = max(transmitTime) + 75 / 1000 (:462-465); pseudorange = (localTime -
 *     transmitTime) * cSpeed (:466); after the fit localTime -= clkBias / cSpeed (recorded, :550-551),
 *     then localTime += measSampleStep / Fs (:554);
 *   - az / el / iono / tropo refresh when counter_corr reaches corrUpt (:489-502), stale values in
 *     between: corrUpt = 10 and counters 9 at the start (:128-130); GNSS_CT_POS_UPDATED: every step
 *     in which any channel runs the 10-ms branch sets corrUpt = 1 and the counters 0 (:301-302)
 *     before that step's epoch, so every 10th epoch until the first channel switches, every epoch
 *     after; GNSS_CT_POS_MULTICORR: corrUpt = 0.01 / (pdi * ms) throughout;
 *   - olspos.m warm-started from the last estusr_wls (first [cnslxyz 0]), tol 1e-3, beta = H \ y by
 *     Householder QR with column pivoting until norm(beta) <= tol (a NaN beta ends the loop as in
 *     MATLAB); the reference has no iteration cap: GNSS_ENOCONV after 50. DOP from inv(H' * H);
 *   - LS_SA_code_Vel.m with lambda = 0.190293672798365 on carrFreq - IF, carrFreq the loop's
 *     current value, i.e. the record at row Index (not index) (:513-514);
 *   - fewer than 4 channels: GNSS_EARG (hmat.m:10). No epoch reached: rows = 0, GNSS_OK.
 * sampleEndMea (:161) is computed by the reference and never used. */
#define GNSS_ENOCONV    6  /* olspos.m's iteration did not converge within 50 steps (the
                              reference has no cap and would spin)                           */
#define GNSS_CT_POS_UPDATED    0
#define GNSS_CT_POS_MULTICORR  1

typedef struct gnss_ct_pos_cfg {
    int32_t n;                  /* channels: the first n of the record set, 4..GNSS_VT_MAX_CH   */
    int32_t mode;               /* GNSS_CT_POS_UPDATED / GNSS_CT_POS_MULTICORR                   */
    int32_t dataType;           /* file.dataType                                                 */
    int32_t msToProcessCT_1ms;  /* track.msToProcessCT_1ms (GNSS_CT_POS_UPDATED)                 */
    int32_t pdi;                /* track.pdi (GNSS_CT_POS_MULTICORR: corrUpt)                    */
    int32_t reserved;
    double  navSolPeriod;       /* solu.navSolPeriod, ms                                         */
    double  Fs, IF, codelength, ms;   /* signal.*                                                */
    double  cSpeed, doy;        /* cmn.cSpeed, cmn.doy                                           */
    double  cnslxyz[3];         /* the first warm start and the ENU origin (:36, :517)           */
    double  ALPHA[4], BETA[4];  /* broadcast iono model (initParameters.m:29-30)                 */
    int32_t countinx[GNSS_VT_MAX_CH];     /* by channel POSITION (:29,183; quirk A.17)           */
    int64_t nav1[GNSS_VT_MAX_CH];         /* sbf.nav1(prn)                                       */
    int64_t sfb1[GNSS_VT_MAX_CH];         /* eph(prn).sfb(1)                                     */
    int64_t sampleStart[GNSS_VT_MAX_CH];  /* TckResult_Eph(prn).absoluteSample(nav1 + sfb1 * 20)
                                             (:156; the caller's mirror reads it)                */
    double  TOW1[GNSS_VT_MAX_CH];         /* eph(prn).TOW(1)                                     */
    gnss_eph_sv eph[GNSS_VT_MAX_CH];      /* ephemeris(prn).*(1) (eph_idx = 1, :126)             */
} gnss_ct_pos_cfg;

/* navSolutionsCT (:509-551), caller-allocated and row-major: `cap` rows per array, `rows` written
 * back. n = gnss_ct_pos_cfg.n values per row where marked [n]. The last four arrays are not in
 * the reference's struct and may be NULL. GNSS_EARG if more than cap epochs fire (one per
 * tracking step at most, so cap = the records' steps always suffices). */
typedef struct gnss_nav_sol_ct {
    int64_t cap;
    int64_t rows;
    double *rawPseudorange;   /* [n] (:509)                                                     */
    double *usrPos;           /* [3] ECEF m                                                     */
    double *usrVel;           /* [3] m/s                                                        */
    double *usrPosENU;        /* [3] about cnslxyz                                              */
    double *usrPosLLH;        /* [3] degrees, degrees, m (:529-530)                             */
    double *clkBias;          /* [1] m                                                          */
    double *usrVelENU;        /* [3]                                                            */
    double *clkDrift;         /* [1] m/s                                                        */
    double *DOP;              /* [4] GDOP PDOP HDOP VDOP (olspos.m:56-61)                       */
    double *satEA;            /* [n] degrees                                                    */
    double *satAZ;            /* [n] degrees                                                    */
    double *timeTransmit;     /* [n] s                                                          */
    double *codePhaseMeas;    /* [n] chips                                                      */
    double *localTime;        /* [1] s, after the clock correction (:550-551)                   */
    int64_t *Index;           /* [1] the tracking step at which the epoch fired (1-based)       */
    int64_t *index;           /* [n] each channel's `index` (:447, 1-based)                     */
    double  *carrFreqMeas;    /* [n] carrFreq(Index), the velocity fit's measurement            */
    int32_t *iters;           /* [1] olspos iterations                                          */
} gnss_nav_sol_ct;

/* The pass. records: the output of gnss_tracking_ct_pos (GNSS_CT_POS_UPDATED) or
 * gnss_tracking_ct_mc (GNSS_CT_POS_MULTICORR), or any array of that layout; read are rec (the
 * absoluteSample, remChip, codeFreq and carrFreq series of channels 0..n-1), max_len, len (the
 * pass runs over min(len) steps) and flags. With GNSS_OUT_DEVICE in records->flags rec is a device
 * pointer of the context's device and the measurement table (Index, index, codePhaseMeas,
 * carrFreq(Index): 4 values per channel and epoch) is extracted on the GPU (csrc/ctpos.hip), so
 * the records never cross PCIe; otherwise on the host. The two tables are equal bit for bit. A
 * record index outside the series, caught by the kernels' bound check, returns GNSS_EDEVICE with
 * the context usable. Host records need no GPU and ctx may be NULL; device records on a context
 * of gnss_ctx_create_multi return GNSS_EARG (no gathering across members). On an error out->rows
 * is 0. */
int gnss_ct_pos_solve(gnss_ctx *ctx, const gnss_ct_pos_cfg *cfg, const gnss_track_out *records,
                      gnss_nav_sol_ct *out);

/* ---- ACF/CalculateFeatures.m (additive within ABI v13; detected by symbol) ----------------
 * The multipath / NLOS features of the 25-tap records, as a pass over the records of
 * gnss_tracking_ct_mc, gnss_tracking_ct_multicorr or a packed trackingVT_..._multicorrelator
 * run. All arithmetic fp64, every operation rounded on its own, every sum left to right. Per
 * channel with L = len rows (line cites of CalculateFeatures.m):
 *   - corr(i, j) = sqrt(I*I + Q*Q) of tap j-1 in storage order, j = 1..25 (:197-225; the order
 *     of :198-224 is the storage order E_060 ... E_005, P, L005 ... L060);
 *   - cenDelay = maxDelay / corrSpacing + 1 in fp64 (:176; 12.999999999999998 for the defaults,
 *     so a prompt peak contributes 8.88e-17 chip, not 0);
 *   - windows m = 1 .. floor((L - ind_start) / numOverLap) (:234; a record whose length is a
 *     multiple of numOverLap loses its last window), sample n of window m is row
 *     r = ind_start - 1 + n + (m - 1) * numOverLap;
 *   - maxCorrInd(m, n) = the first index of the largest corr(r, :) (:236; a NaN counts as
 *     missing, an all-NaN row gives 1); maxCorr(n) = corr(r, 13), the prompt magnitude, which
 *     overwrites the maximum (:237);
 *   - tmpDelay(n) = (maxCorrInd(m, n) - mean(maxCorrInd(m, :))) * corrSpacing with the mean over
 *     the row as it stands at that moment (:238): S_n / n in a channel's first window (the row
 *     grows; maxCorrInd is cleared per PRN, :294), S_n / numOverLap in every later one (the row
 *     is already numOverLap wide and zero filled), S_n the exact sum of the first n indices;
 *   - meanMax = sum(maxCorr) / numOverLap (:260), meanDelay = sum((maxCorrInd(m, :) - cenDelay) *
 *     corrSpacing) / numOverLap (:270), varDelay = sum(tmpDelay.^2) / numOverLap (:271),
 *     meanCodeDisc = mean(d), varCodeDisc = var(d) (:273-274; two passes, n - 1 below) with d the
 *     GNSS_F_DLLdiscri (= codeError) series of the window's rows;
 *   - F1 = meanMax / expectedCorr, expectedCorr = a[0] + a[1]*ele + a[2]*ele^2 + a[3]*ele^3 left
 *     to right with pow (:186-188); F2 = -(meanDelay + 0.00) * 1 (:279).
 * The plotting tail (:298-323) is not part of it. The reference ships no output of this script:
 * the definition is this restatement. */
typedef struct gnss_acf_cfg {
    int32_t n;                  /* channels: the first n of the record set, 1..GNSS_VT_MAX_CH */
    int32_t ind_start;          /* :178, 1-based; default 1                                   */
    int32_t numOverLap;         /* :179, rows per window, 2..4096; default 100                */
    int32_t reserved;
    double  corrSpacing;        /* :173, default 0.05                                         */
    double  maxDelay;           /* :174, default 0.6                                          */
    double  a[4];               /* :186, default 4092.9779845217 340.423503277404
                                   -2.99026922880033 0.0251763660254827                       */
    int32_t prn[GNSS_VT_MAX_CH];/* prnList, echoed by the caller's data_labeled               */
    double  ele[GNSS_VT_MAX_CH];/* eleList, degrees                                           */
} gnss_acf_cfg;

/* Caller-allocated. The six feature arrays are row-major [n][cap] host arrays; channel c's
 * window m (0-based) is at [c * cap + m], windows[c] of them written. maxCorrInd and corr are
 * optional (NULL: not wanted) and cover every row i < len[c] of a channel, in a window or not:
 * maxCorrInd[c * max_len + i] is the 1-based arg-max of row i, corr[(c * 25 + j) * max_len + i]
 * the magnitude of tap j. With GNSS_OUT_DEVICE in records->flags these two are DEVICE pointers
 * (they are as large as the records), otherwise host pointers. */
typedef struct gnss_acf_out {
    int64_t  cap;             /* windows per channel the arrays hold                          */
    int64_t *windows;         /* [n]                                                          */
    double  *meanMax;         /* mean prompt magnitude (:260)                                 */
    double  *F1;              /* meanMax / expectedCorr (:278)                                */
    double  *F2;              /* -(meanDelay + 0.00) * 1, chips (:279)                        */
    double  *varDelay;        /* F3 (:271)                                                    */
    double  *meanCodeDisc;    /* F4 (:273)                                                    */
    double  *varCodeDisc;     /* F5 (:274)                                                    */
    uint8_t *maxCorrInd;      /* [n][max_len], 1..25; may be NULL                             */
    double  *corr;            /* [n][25][max_len]; may be NULL                                */
} gnss_acf_out;

/* The pass. records: rec (the GNSS_F_DLLdiscri series), taps [nsv][2][25][max_len], len,
 * max_len and flags are read; n_taps is the records' tap count and must be GNSS_MC_TAPS. Host
 * records need no GPU and ctx may be NULL; with GNSS_OUT_DEVICE rec and taps are device pointers
 * of the context's device and the pass runs on the GPU (csrc/acf.hip): one streaming pass over
 * the taps, only the features cross PCIe. Both paths give the same bits in every output. Device
 * records on a context of gnss_ctx_create_multi return GNSS_EARG. GNSS_EARG also for n_taps !=
 * 25, n outside 1..GNSS_VT_MAX_CH, numOverLap outside 2..4096, ind_start < 1, corrSpacing <= 0,
 * len[c] outside 0..max_len and more windows than cap: all checked on the host before any
 * launch, so no kernel indexes past len[c] rows of a max_len series. */
int gnss_acf_features(gnss_ctx *ctx, const gnss_acf_cfg *cfg, const gnss_track_out *records,
                      int32_t n_taps, gnss_acf_out *out);

/* ---- CalculateFeatures.m's F6-F8 (additive within ABI v13; detected by symbol) -------------
 * The three features the script keeps behind comment marks; its data sets were once 11 columns
 * wide (:32). They look at how a channel's correlation changes from window to window: a
 * reflected ray's carrier turns against the direct one's, so the prompt magnitude fades at the
 * ray's Doppler difference. All arithmetic fp64, every operation rounded on its own (no
 * contraction, no fast-math), every sum left to right from its first term (csrc/acf_ext.h is the
 * one source for host and device). Windows, rows and corr(i, j) are gnss_acf_features': row m of
 * channel c lines up with that call's rows, with gnss_acf_fit's and with the scene's labels.
 *   - F6 numMLC(m): cnt(r) = the number of columns j = 2..24 (1-based) of row r with
 *     corr(r, j) > corr(r, j-1) && corr(r, j) > corr(r, j+1) (:247-251). The edge columns never
 *     count (the commented edge tests of :244-246 and :252-254 stay off), a plateau of equal
 *     values counts nothing, a NaN compares false. numMLC(m) = (the exact integer sum of cnt over
 *     the window's rows) / numOverLap, one division (:256).
 *   - History: per channel a buffer of fft_hist values (:231, 300), all zero at the channel's
 *     start (:293 resets it per PRN); at window m it is shifted left by one and meanMax(m) is
 *     appended (:262). x[i], i = 0..H-1, is the buffer oldest first, H = fft_hist:
 *     x[i] = meanMax(m - H + 1 + i), or 0 where that window lies before the channel's first. So a
 *     record shorter than fft_hist windows (30 s with the defaults) mostly shows the step from
 *     the zero fill. fft_fill = 1 is the one departure on offer: only the windows that exist
 *     are taken, H = min(m + 1, fft_hist), no zero entries. Default 0, the script's form.
 *   - Spectrum (:263-268): mean = (sum of x[i]) / H, y[i] = x[i] - mean; for k = 0..floor(N/2),
 *     N = fft_n (:264, 1024), t = (k*i) mod N: re = sum_i y[i]*c[t], im = sum_i y[i]*s[t],
 *     mag[k] = sqrt(re*re + im*im), with c[t] = cos((2*pi*t)/N) and s[t] = sin((2*pi*t)/N) from
 *     one table that the host builds once per call with the C library (gnss_acf_twiddle returns
 *     it); both paths read it, the device gets it uploaded. The script's fft has the other sign
 *     of im, which mag does not see. The search stops at N/2: the upper bins of a real series
 *     mirror the lower ones, and MATLAB's first-index max never picks them in exact arithmetic;
 *     in rounded arithmetic a mirror bin could come out an ulp larger there, never here.
 *   - I = the first index of the largest mag, 1-based, scanned as maxCorrInd is: from -1, taken
 *     on v > best, a NaN as missing; if every bin is NaN (a NaN meanMax in the history), I = 1
 *     and M = NaN. fftFreq = ((I-1)*fs)/N (:267), fftMag = M/(N/2) (:268): the script divides by
 *     N/2 whatever H is, and so does this. */
typedef struct gnss_acf_ext_cfg {
    int32_t fft_hist;           /* :231, 2..512; default 300                                  */
    int32_t fft_n;              /* :264, fft_hist..2048; default 1024                         */
    int32_t fft_fill;           /* 0: zero-filled history (the script), 1: existing windows   */
    int32_t reserved;
    double  fs;                 /* :172, windows per second: 1000 / (numOverLap * pdi)        */
} gnss_acf_ext_cfg;

/* Caller-allocated host arrays, row-major [n][out->cap] each, as gnss_acf_out's six. */
typedef struct gnss_acf_ext_out {
    double *numMLC;           /* F6 (:256)                                                    */
    double *fftFreq;          /* F7, Hz (:267)                                                */
    double *fftMag;           /* F8 (:268)                                                    */
} gnss_acf_ext_out;

/* gnss_acf_features with F6-F8 beside it: everything that call does, `out` equal to that call's
 * bit for bit (maxCorrInd and corr included), and ext filled as well. The same rules: host
 * records need no GPU and ctx may be NULL; GNSS_OUT_DEVICE records run on the GPU (the row pass
 * of csrc/acf.hip also writes cnt(r), one byte per row; csrc/acf_ext.hip, one block per window,
 * forms the spectrum from the windows' meanMax in device memory); device records on a context of
 * gnss_ctx_create_multi return GNSS_EARG. Both paths give the same bits in every output.
 * GNSS_EARG also for everything gnss_acf_features refuses and for fft_hist outside 2..512, fft_n
 * outside fft_hist..2048, fft_fill not 0 or 1, fs not finite or <= 0 and a null array: all
 * checked on the host before any launch, the context usable after. gnss_acf_features itself is
 * unchanged. */
int gnss_acf_features_ext(gnss_ctx *ctx, const gnss_acf_cfg *cfg, const gnss_acf_ext_cfg *ext_cfg,
                          const gnss_track_out *records, int32_t n_taps, gnss_acf_out *out,
                          gnss_acf_ext_out *ext);

/* The table both paths read: c[t] = cos((2*pi*t)/fft_n), s[t] = sin(...), t = 0..fft_n-1, from
 * the C library. GNSS_EARG for fft_n outside 2..2048 or a null array. */
int gnss_acf_twiddle(int32_t fft_n, double *c, double *s);

/* ---- two-path fit of the 25-tap ACF (additive within ABI v13; detected by symbol) ---------
 * A multipath delay estimate per feature window: a direct path plus one reflected path fitted to
 * the coherently summed 25-tap correlation function. It goes beyond the reference, which has no
 * such estimator. All arithmetic fp64, every operation rounded on its own, every sum left to
 * right from its first term (csrc/acf_fit.h is the kernel's source; the host path runs the same
 * functions at 25 taps from csrc/acf_fit_taps.h).
 *   - Windows: gnss_acf_features' (ind_start, numOverLap, the same count and rows), so fit row m
 *     of channel c lines up with feature row m.
 *   - Coherent vector: for row r of the window s_r = +1 if the prompt's I sum (tap 12 of 0..24) is
 *     >= 0, else -1 (a NaN gives -1); zI[j] = sum_r s_r*I[j][r], zQ[j] = sum_r s_r*Q[j][r], rows
 *     ascending; energy = sum_j (zI[j]*zI[j] + zQ[j]*zQ[j]).
 *   - Tap coordinate u[j] = (orient * (j - 12)) * corrSpacing. With orient = +1 a path that
 *     arrives later sits at a lower u (the records of gnss_tracking_ct_multicorr); the 10-ms
 *     loop of gnss_tracking_ct_mc and the vector loop store their taps the other way: -1.
 *   - Model R(x) = max(0, 1 - |x|). Grid p = p_min + ip*p_step, e = e_min + ie*e_step.
 *   - One path, per ip with r_j = R(u[j] - p): a = sum r_j*r_j (skipped if a == 0),
 *     A = (sum r_j*z_j) / a per component, res = sum_j |z_j - A*r_j|^2 as dI*dI + dQ*dQ. The
 *     smallest res wins, the lowest ip on a tie; a NaN res never wins.
 *   - Two paths, h = ip*e_count + ie, r0_j = R(u[j] - p), r1_j = R(u[j] - (p - e)): a = sum r0*r0,
 *     b = sum r1*r1, c = sum r0*r1, h0 = sum r0*z, h1 = sum r1*z, det = a*b - c*c; skipped if
 *     a == 0, b == 0 or !(det > (1e-9*a)*b) (a path outside the tap span);
 *     A0 = (b*h0 - c*h1)/det, A1 = (a*h1 - c*h0)/det; skipped if |A1|^2 > (ratio_max*ratio_max) *
 *     |A0|^2 (a reflection above the direct path is the NLOS case and belongs to the one-path
 *     fit); res = sum_j |(z_j - A0*r0_j) - A1*r1_j|^2. The smallest (res, h) wins.
 *   - paths = 2 iff a two-path hypothesis survived and res1 > gain_min*res2, else 1; paths = 0
 *     (every output of the window NaN) for a non-finite z or when no one-path hypothesis
 *     survived. bias = p of the selected model, chips: how late the prompt is against the direct
 *     path. A0 is the direct path, A1 the reflected one, e > 0 its excess delay in chips. */
typedef struct gnss_acf_fit_cfg {
    int32_t n;                  /* channels: the first n of the record set, 1..GNSS_VT_MAX_CH */
    int32_t ind_start;          /* as gnss_acf_cfg; default 1                                 */
    int32_t numOverLap;         /* rows per window, 2..4096; default 100                      */
    int32_t orient;             /* +1 or -1 (above)                                           */
    double  corrSpacing;        /* default 0.05                                               */
    double  p_min, p_step;      /* default -0.40, 0.01                                        */
    double  e_min, e_step;      /* default 0.05, 0.01                                         */
    int32_t p_count, e_count;   /* default 81, 96; each >= 1, p_count*e_count <= 65536        */
    double  ratio_max;          /* default 1.0                                                */
    double  gain_min;           /* default 16.0                                               */
} gnss_acf_fit_cfg;

/* Caller-allocated host arrays, row-major [n][cap]: channel c's window m (0-based) is at
 * [c * cap + m], windows[c] of them written. zI and zQ are optional (NULL: not wanted):
 * [(c * 25 + j) * cap + m] is tap j of the window's coherent vector. */
typedef struct gnss_acf_fit_out {
    int64_t  cap;             /* windows per channel the arrays hold                          */
    int64_t *windows;         /* [n]                                                          */
    int32_t *paths;           /* 0, 1 or 2                                                    */
    double  *bias;            /* chips                                                        */
    double  *p1, *A1p_re, *A1p_im, *res1;                       /* the one-path fit           */
    double  *p0, *e, *A0_re, *A0_im, *A1_re, *A1_im, *res2;     /* the two-path fit, or NaN   */
    double  *energy;
    double  *zI, *zQ;         /* [n][25][cap]; may be NULL                                    */
} gnss_acf_fit_out;

/* The fit over a record set. records: taps [nsv][2][25][max_len], len, max_len and flags are
 * read; n_taps must be GNSS_MC_TAPS. Host records need no GPU and ctx may be NULL (up to 16
 * threads); with GNSS_OUT_DEVICE taps is a device pointer of the context's device and the fit
 * runs on the GPU (csrc/acf_fit.hip), one block per window. Both paths give the same bits in
 * every output. Device records on a context of gnss_ctx_create_multi return GNSS_EARG. GNSS_EARG
 * also for n_taps != 25, n outside 1..GNSS_VT_MAX_CH, numOverLap outside 2..4096, ind_start < 1,
 * orient not +-1, corrSpacing, p_step or e_step not positive, a non-finite p_min or e_min, a count
 * below 1, p_count*e_count > 65536, a ratio_max or gain_min that is negative or NaN, len[c]
 * outside 0..max_len and more windows than cap: all checked on the host before any launch. */
int gnss_acf_fit(gnss_ctx *ctx, const gnss_acf_fit_cfg *cfg, const gnss_track_out *records,
                 int32_t n_taps, gnss_acf_fit_out *out);

/* The fit alone on one coherent vector zI[25], zQ[25], host only: cfg's orient, corrSpacing, grid
 * and thresholds are read (n, ind_start and numOverLap are not); out is a gnss_acf_fit_out with
 * cap >= 1 whose element [0] of every array is written (windows[0] = 1; zI / zQ, if given, get
 * the vector at [j * cap]). For known-answer tests and for a caller that forms z differently. */
int gnss_acf_fit_window(const gnss_acf_fit_cfg *cfg, const double *zI, const double *zQ,
                        gnss_acf_fit_out *out);

/* ---- k-NN classifier over the feature windows (additive within ABI v13; detected by symbol) --
 * ACF/CalculateFeatures.m names its table data_labeled: a training set for a classifier that
 * says, per 100-ms window, line of sight / multipath / no direct signal (0 / 1 / 2, the labels of
 * a synthetic scene). A brute-force k-nearest-neighbour vote on standardised columns; it goes
 * beyond the reference, which stops at the table. All arithmetic fp64, every operation rounded on
 * its own, every sum left to right from its first term (csrc/knn.h is the one source for host
 * and device).
 *   - Standardisation of x[M][D]: mu[j] = (sum_t x[t][j]) / M, var[j] = (sum_t (x[t][j] - mu[j]) *
 *     (x[t][j] - mu[j])) / M, sd[j] = sqrt(var[j]), inv[j] = 1 / sd[j] or 0 when sd[j] == 0 (a
 *     constant column drops out of every distance), z[t][j] = (x[t][j] - mu[j]) * inv[j].
 *   - Query q[D]: zq[j] = (q[j] - mu[j]) * inv[j], d2(t) = sum_j (zq[j] - z[t][j]) * (zq[j] -
 *     z[t][j]), j ascending. A query with a non-finite q[j] (the raw value: also on a column
 *     with inv[j] = 0) gets label -1, all votes 0, every neighbour index -1 and d2 NaN.
 *   - Neighbours: the k smallest training rows under the total order (d2, t): the smaller d2
 *     first, on equal d2 the smaller row; +inf is an ordinary value and a NaN d2 (a finite query
 *     so far out that q[j] - mu[j] overflows on a constant column) comes after it, stored as the
 *     quiet NaN 0x7ff8000000000000. Returned ascending in that order.
 *   - votes[c]: the neighbours of class c; label: the class with the most votes, among tied
 *     classes the one that owns the nearest neighbour.                                        */
#define GNSS_KNN_HOST         1  /* gnss_knn_cfg.flags: the host path also with a context      */
#define GNSS_KNN_MODEL_DEVICE 1  /* gnss_knn_model.flags: z and label are DEVICE pointers of the
                                    context's device (gnss_dev_alloc / gnss_dev_upload)        */
typedef struct gnss_knn_cfg {
    int32_t k;                /* neighbours, 1..32 and <= M                                    */
    int32_t flags;            /* GNSS_KNN_HOST or 0                                            */
} gnss_knn_cfg;

typedef struct gnss_knn_model {
    int64_t        M;         /* training rows, 1..2^24                                        */
    int32_t        D;         /* columns, 1..16                                                */
    int32_t        n_class;   /* classes, 1..8                                                 */
    const double  *mu, *inv;  /* [D], host                                                     */
    const double  *z;         /* [M][D] standardised rows                                      */
    const int32_t *label;     /* [M], each in 0..n_class-1                                     */
    int32_t        flags;     /* GNSS_KNN_MODEL_DEVICE or 0                                    */
    int32_t        reserved;
} gnss_knn_model;

/* Caller-allocated host arrays. nn_index and nn_d2 are optional (NULL: not wanted). */
typedef struct gnss_knn_out {
    int32_t *label;           /* [Q]                                                           */
    int32_t *votes;           /* [Q][n_class]                                                  */
    int32_t *nn_index;        /* [Q][k] training rows, nearest first; may be NULL              */
    double  *nn_d2;           /* [Q][k]; may be NULL                                           */
} gnss_knn_out;

/* mu[D], inv[D] and z[M][D] of the training table x[M][D] (above). Host only. GNSS_EARG for a
 * null array, M outside 1..2^24, D outside 1..16, a non-finite x or a non-finite mu, sd or inv. */
int gnss_knn_standardize(const double *x, int64_t M, int32_t D, double *mu, double *inv, double *z);

/* Q query rows q[Q][D] (host, raw) against the model. ctx == NULL or GNSS_KNN_HOST: on the host,
 * the queries dealt over up to 16 threads. Otherwise on the GPU (csrc/knn.hip): q and the outputs
 * stay host arrays; model->z and model->label are host arrays that the call uploads, or with
 * GNSS_KNN_MODEL_DEVICE device arrays that stay where they are (a caller that classifies many
 * record sets uploads the model once). Both paths give the same bits in every output. Checked on
 * the host before any launch, GNSS_EARG otherwise and the context usable after: D in 1..16, k in
 * 1..32 and <= M, n_class in 1..8, every training label in 0..n_class-1, M in 1..2^24, Q >= 0
 * (Q == 0: GNSS_OK, nothing written), no null array that is not optional, no unknown flag, a
 * device model only with a context and the device path, and no context of gnss_ctx_create_multi
 * on the device path. */
int gnss_knn_classify(gnss_ctx *ctx, const gnss_knn_cfg *cfg, const gnss_knn_model *model,
                      const double *q, int64_t Q, gnss_knn_out *out);

/* ---- replay correlator (additive within ABI v13; detected by symbol) -----------------------
 * Recorded tracking rows correlated again on any tap grid, with no loop closed. Every 25-tap loop
 * freezes its taps at -0.6:0.05:0.6 chip when it runs; a reflected ray later than that is outside
 * every record. A row's correlation, though, is fixed by the NCO state the loop left after the row
 * before it and by the row's own read: row i starts at byte absoluteSample(i-1) with
 * remChip(i-1), codeFreq(i-1), carrierFreq(i-1), remPhase(i-1) and reads numSample(i) samples
 * (row 0: the loop's initial state and seek). Replayed with the loop's own taps a row returns the
 * recorded sums; with other taps it shows the correlation function wherever the caller looks.
 * Rows are independent of each other, so the GPU path (csrc/replay.hip) has one workgroup per
 * (row, channel, tile of 32 taps) and no hand-off between workgroups.
 *
 * Per row and tap s (correlate_cpx of the reference loops, trackingCT.m:96-118):
 *   d = codeFreq / Fs; tap s's time axis is MATLAB's colon
 *   ((0 + tap[s]) + remChip) : d : (((n-1)*d + tap[s]) + remChip), which must have exactly n
 *   elements (else GNSS_EINDEX, the error text naming channel, row and tap); t = element k, plus
 *   post[s] if post is given; chip CA[(ceil(t) + chip_off + 1022) mod 1023] with a true modulus, so
 *   any finite tap works. chip_off = 0 is Code(ceil(t)+1) of trackingCT.m and
 *   trackingCT_multiCorr-GIVEN.m, chip_off = 1 Code(ceil(t)+2) of the two _POS siblings. Inside the
 *   reference's padded code tables this is the chip they hold; outside it is the code's PERIODIC
 *   EXTENSION, without the data bit's flips (a tap far from the prompt crosses bit edges the
 *   replica does not know).
 *   Carrier: Wave(k) = 2*pi*(carrFreq*(k/Fs)) + remPhase with the reference's roundings,
 *   I = xr*sin + xi*cos, Q = xr*cos - xi*sin, summed in fp64 in a fixed order.
 * A tap offset delays the REPLICA, so a ray that arrives tau chips late shows at tap -tau: the
 * delayed ray appears at negative taps (as in the 25-tap records of the GIVEN loop).
 * Records are int8, dataType 2 (I/Q pairs) or 1 (real, xi = 0); int16 records: GNSS_EARG.
 * A row's bits depend on that row alone: not on the other rows or channels of the call, on host or
 * device output, on how the call was segmented (gnss_ctx_set_window), or on the run (no float
 * atomics). The host path and the GPU path sum in different orders and agree to rounding. */
#define GNSS_REPLAY_MAX_TAPS 256
typedef struct gnss_replay_cfg {
    int32_t       n_taps;       /* 1..GNSS_REPLAY_MAX_TAPS                                      */
    int32_t       chip_off;     /* 0 or 1                                                       */
    const double *tap_offsets;  /* [n_taps] chips, finite, |tap| <= 1023                        */
    const double *post;         /* [n_taps] added to a tap's element before ceil (the +0.05 of
                                   trackingCT_POS_updated.m:216), |post| <= 1023; NULL = none   */
    int32_t       flags;        /* GNSS_OUT_DEVICE: out->taps is a DEVICE pointer, or 0         */
    int32_t       reserved;
} gnss_replay_cfg;

/* The rows' NCO states, [n_chan][max_rows] arrays of which channel c uses rows 0..n_rows[c]-1. */
typedef struct gnss_replay_rows {
    int32_t        n_chan;      /* 1..GNSS_MAX_SV                                               */
    int32_t        reserved;
    int64_t        max_rows;
    const int32_t *prn;         /* [n_chan] 1..51                                               */
    const int64_t *n_rows;      /* [n_chan] 0..max_rows (0: the channel sits the call out)      */
    const int64_t *pos_bytes;   /* the row's first file byte                                    */
    const int64_t *numSample;   /* samples read, 1..2^22                                        */
    const double  *remChip;     /* at the row's start                                           */
    const double  *codeFreq;    /* > 0; (numSample-1) * codeFreq / Fs at most 2^28 chips        */
    const double  *carrFreq;
    const double  *remPhase;
} gnss_replay_rows;

typedef struct gnss_replay_out {
    double *taps;       /* [n_chan][2][n_taps][max_rows], gnss_track_out.taps' layout: I then Q;
                           rows >= n_rows[c] are left untouched                                 */
    double  kernel_ms;  /* out: hipEvents around the kernel(s); 0 on the host path              */
} gnss_replay_out;

/* ctx == NULL: the host path (up to 16 threads, the rows dealt over them; the bits do not depend on
 * the thread count), the record from file->data or file->path. Otherwise the GPU: the bytes
 * [min pos_bytes, max row end) are staged into HBM (a dev_data record is read where it lies); if
 * they exceed the context's window (gnss_ctx_set_window) the rows are processed in consecutive
 * segments, each staging its own range (GNSS_EARG if one row index of all channels does not fit;
 * gnss_last_timing's track_segments then holds the segment count, h2d_ms / h2d_bytes the staging).
 * Everything is checked on the host before any launch and every refusal leaves the context usable
 * and the output untouched: GNSS_EARG for a null argument, n_taps, chip_off, a tap or post value,
 * an unknown flag, n_chan, a PRN, n_rows, numSample outside 1..2^22, a non-finite state, codeFreq,
 * an int16 record, GNSS_OUT_DEVICE without a context or with taps that is not device memory of
 * the context's device, or a context of gnss_ctx_create_multi; GNSS_EIO for pos_bytes < 0, not a
 * multiple of the sample size, or a read past the record's end; GNSS_EINDEX for a colon that has
 * not numSample elements. */
int gnss_replay_correlate(gnss_ctx *ctx, const gnss_file *file, const gnss_signal *signal,
                          const gnss_replay_cfg *cfg, const gnss_replay_rows *rows,
                          gnss_replay_out *out);

/* ---- two-path fit of an ACF on any tap grid (additive within ABI v13; detected by symbol) ---
 * gnss_acf_fit's estimator for the sums gnss_replay_correlate writes: a reflected ray whose
 * triangle lies outside the 25 taps' +-0.6 chip can be replayed on a wider grid and then fitted.
 * The definition is gnss_acf_fit's (the comment above gnss_acf_fit_cfg) with three substitutions
 * and nothing else (csrc/acf_fit_taps.h is the one source for host and device):
 *   - 25 becomes n_taps, 1..GNSS_REPLAY_MAX_TAPS;
 *   - the prompt index 12 becomes `prompt`, 0..n_taps-1: the tap whose I sum of the same row
 *     gives the row's sign s_r (>= 0: +1, otherwise -1; a NaN gives -1);
 *   - u[j] = (orient*(j-12))*corrSpacing becomes u[j] as the caller gives it: finite, in any
 *     order, uniform or not, in orient = +1's convention (a path that arrives later sits at a
 *     lower u). For replayed sums u = tap_offsets as they are.
 * The windows, the first row's term taken as it is, every sum left to right from its first term
 * over all n_taps taps, the skip rules, the smallest (res, index), paths = 0 / 1 / 2 and the NaN
 * outputs carry over. With n_taps = 25, prompt = 12 and u[j] = (orient*(j-12))*corrSpacing every
 * output equals gnss_acf_fit's bit for bit, on the host and on the GPU. */
typedef struct gnss_acf_fit_taps_cfg {
    int32_t       n;            /* channels, 1..GNSS_VT_MAX_CH                                  */
    int32_t       ind_start;    /* as gnss_acf_cfg, >= 1; default 1                             */
    int32_t       numOverLap;   /* rows per window, 2..4096; default 100                        */
    int32_t       n_taps;       /* 1..GNSS_REPLAY_MAX_TAPS                                      */
    int32_t       prompt;       /* 0..n_taps-1                                                  */
    int32_t       flags;        /* GNSS_OUT_DEVICE: in->taps is a DEVICE pointer, or 0          */
    const double *u;            /* [n_taps] tap coordinates in chips, host, finite              */
    double        p_min, p_step;      /* default -0.40, 0.01                                    */
    double        e_min, e_step;      /* default 0.05, 0.01                                     */
    int32_t       p_count, e_count;   /* default 81, 196; each >= 1, p_count*e_count <= 65536   */
    double        ratio_max;    /* default 1.0                                                  */
    double        gain_min;     /* default 16.0                                                 */
} gnss_acf_fit_taps_cfg;

typedef struct gnss_acf_fit_taps_in {
    const double  *taps;        /* [n][2][n_taps][max_rows], gnss_replay_out.taps' layout: a host
                                   array, or with GNSS_OUT_DEVICE device memory of the context's
                                   device                                                       */
    int64_t        max_rows;    /* >= 1                                                         */
    const int64_t *n_rows;      /* [n] host, each 0..max_rows: channel c's windows lie below it */
} gnss_acf_fit_taps_in;

/* The fit over replayed sums. out: gnss_acf_fit's struct, zI / zQ (optional) [n][n_taps][cap].
 * Host sums need no GPU and ctx may be NULL (up to 16 threads, a window by one thread: the bits do
 * not depend on the thread count); with GNSS_OUT_DEVICE the fit runs on the GPU
 * (csrc/acf_fit_taps.hip, one block per window) and gnss_last_timing's track_kernel_ms holds the
 * kernel's duration. Both paths give the same bits in every output. Everything is checked on the
 * host before any launch; each refusal sets the error text and leaves the outputs untouched and
 * the context usable. GNSS_EARG for a null argument, n, n_taps or prompt out of range, a
 * non-finite u[j], numOverLap outside 2..4096, ind_start < 1, p_step or e_step not positive, a
 * non-finite p_min or e_min, a count below 1, p_count*e_count > 65536, a ratio_max or gain_min
 * that is negative or NaN, max_rows < 1, n_rows[c] outside 0..max_rows, more windows than cap, an
 * unknown flag, GNSS_OUT_DEVICE without a context or with taps that is not device memory of the
 * context's device, and device sums on a context of gnss_ctx_create_multi. */
int gnss_acf_fit_taps(gnss_ctx *ctx, const gnss_acf_fit_taps_cfg *cfg,
                      const gnss_acf_fit_taps_in *in, gnss_acf_fit_out *out);

/* The fit alone on one coherent vector zI[n_taps], zQ[n_taps], host only: cfg's n_taps, u, grid
 * and thresholds are read (n, ind_start, numOverLap, prompt beyond its range check and flags are
 * not); out as for gnss_acf_fit_window, zI / zQ, if given, get the vector at [j * cap]. */
int gnss_acf_fit_taps_window(const gnss_acf_fit_taps_cfg *cfg, const double *zI, const double *zQ,
                             gnss_acf_fit_out *out);

/* ---- delay-Doppler map over replayed rows (additive within ABI v14; detected by symbol) -------
 * gnss_replay_correlate gives per-row complex sums on any tap grid with no loop closed, and a
 * window's rows are contiguous in time. Summed coherently with one rotation per row they give the
 * correlation the loop would have seen with its carrier nu Hz higher; for every (tap, nu) cell
 * that is the delay-Doppler map of the window. A reflected ray whose carrier is offset from the
 * direct one (gnss_synth_ray.fade_hz) rotates within the window and cancels in the zero-offset sum
 * that gnss_acf_fit_taps fits; in the map it stands at (its delay, its offset), with the sign.
 * csrc/replay_ddm.h is the one source of the arithmetic for host and device.
 *
 * Per channel c and window w of R = rows_per_window consecutive rows i0 = w*R .. i0+R-1 (only
 * whole windows below n_rows[c] count), one value per tap j and per Doppler offset nu_m [Hz]:
 *   - row time: s_i = (pos_bytes[i] - pos_bytes[i0]) / bytes_per_sample in int64,
 *     t_i = ((double)(2*s_i + numSample[i] - 1) / 2.0) / Fs: the row's middle sample, in seconds
 *     from the window's first sample. The host forms t once; both paths read that table.
 *   - rotation: th = nu_m * t_i, r = th - rint(th), (sn, cs) = sin, cos of kRpTwoPi * r by
 *     csrc/replay.h's rp_sincos; every operation rounds on its own (no contraction).
 *   - sign: s_i from tap `prompt`'s I of the same row: >= 0 gives +1, anything else -1 (a NaN
 *     gives -1): gnss_acf_fit_taps' rule. prompt = -1: no sign wipe (s_i = +1).
 *   - cell: two plain left-to-right sums over the window's rows, ascending i, starting from 0:
 *       ZI += s_i*(I*cs + Q*sn),  ZQ += s_i*(Q*cs - I*sn)
 *     (s_i = +-1 is applied to I and Q first: the same bits, negation being exact). That is
 *     (I + iQ) * exp(-i*2*pi*nu*t). The replay's wipe is I + iQ = i*conj(x*exp(iW)), so the cell is
 *     the rows' sum with carrFreq + nu in place of carrFreq, the rotation held at each row's
 *     middle sample. The loss inside a row is sinc(nu * T_row): 20 Hz on 1-ms rows loses 0.07 %.
 *   - power: P = ZI*ZI + ZQ*ZQ, two rounded products and one add.
 *   - peaks per window: cells are numbered bin-major, k = m*n_taps + j; a cell whose P is a NaN is
 *     no candidate. The peak is the largest P, the lowest k among equals: peak_bin, peak_tap,
 *     peak_pow. The secondary peak is the same rule over the cells with
 *     |u[j] - u[peak_tap]| >= excl_chips OR |dopp_hz[m] - dopp_hz[peak_bin]| >= excl_hz:
 *     sec_bin, sec_tap, sec_pow. No candidate: -1, -1, NaN.
 * The sum order is fixed by the definition, not by the tiling: host and GPU give the same bits in
 * every output, for any thread count, and a window's bits depend on that window alone. */
#define GNSS_DDM_MAX_DOPP   256
#define GNSS_DDM_MAP_DEVICE 2   /* with GNSS_OUT_DEVICE: out->map is DEVICE memory and stays there */
typedef struct gnss_replay_ddm_cfg {
    int32_t       n;                /* channels, 1..GNSS_MAX_SV                                 */
    int32_t       n_taps;           /* 1..GNSS_REPLAY_MAX_TAPS                                  */
    int32_t       prompt;           /* -1 (no sign wipe) or 0..n_taps-1                         */
    int32_t       rows_per_window;  /* 2..4096                                                  */
    int32_t       n_dopp;           /* 1..GNSS_DDM_MAX_DOPP                                     */
    int32_t       flags;            /* 0, GNSS_OUT_DEVICE (in->taps is a DEVICE pointer), or
                                       GNSS_OUT_DEVICE | GNSS_DDM_MAP_DEVICE                    */
    const double *dopp_hz;          /* [n_dopp] host, finite, |nu| <= 1e5, in any order         */
    const double *u;                /* [n_taps] host, tap coordinates in chips, finite          */
    double        excl_chips;       /* >= 0                                                     */
    double        excl_hz;          /* >= 0                                                     */
    double        Fs;               /* > 0, finite                                              */
    int32_t       bytes_per_sample; /* 1 or 2 (the record's dataType at int8)                   */
    int32_t       reserved;
} gnss_replay_ddm_cfg;

typedef struct gnss_replay_ddm_in {
    const double  *taps;        /* [n][2][n_taps][max_rows], gnss_replay_out.taps' layout: a host
                                   array, or with GNSS_OUT_DEVICE device memory of the context's
                                   device                                                       */
    int64_t        max_rows;    /* >= 1                                                         */
    const int64_t *n_rows;      /* [n] host, each 0..max_rows                                   */
    const int64_t *pos_bytes;   /* [n][max_rows] host: gnss_replay_rows' arrays                 */
    const int64_t *numSample;   /* [n][max_rows] host, 1..2^22 in the rows of whole windows     */
} gnss_replay_ddm_in;

typedef struct gnss_replay_ddm_out {
    int64_t  cap;        /* windows per channel the arrays hold                                 */
    double  *map;        /* [n][cap][2][n_dopp][n_taps]: ZI then ZQ; NULL: peaks only. Device
                            memory of the context's device with GNSS_DDM_MAP_DEVICE             */
    int32_t *peak_bin;   /* [n][cap] each of the six; windows >= n_win[c] are left untouched    */
    int32_t *peak_tap;
    double  *peak_pow;
    int32_t *sec_bin;
    int32_t *sec_tap;
    double  *sec_pow;
    int64_t *n_win;      /* [n] out: n_rows[c] / rows_per_window                                */
    double   kernel_ms;  /* out: hipEvents around the kernels; 0 on the host path               */
} gnss_replay_ddm_out;

/* Host sums need no GPU and ctx may be NULL: up to 16 threads, a window by one thread. With
 * GNSS_OUT_DEVICE the map is formed on the GPU (csrc/replay_ddm.hip: one workgroup per window,
 * tile of bins and tile of taps, then one per window for the peaks) and downloaded, or left in
 * out->map with GNSS_DDM_MAP_DEVICE. Everything is checked on the host before any launch; a
 * refusal sets the error text and leaves the outputs untouched and the context usable.
 * GNSS_EARG: a null argument (map excepted), n, n_taps, prompt, rows_per_window or n_dopp out of
 * range, a non-finite u[j] or dopp_hz[m], |dopp_hz[m]| > 1e5, a negative or NaN excl_chips or
 * excl_hz, Fs, bytes_per_sample, max_rows < 1, cap < 0, n_rows[c] outside 0..max_rows, more
 * windows than cap, numSample outside 1..2^22 in a window's row, an unknown flag,
 * GNSS_DDM_MAP_DEVICE without GNSS_OUT_DEVICE or without a map, GNSS_OUT_DEVICE without a context
 * or with taps (or the device map) that is not device memory of the context's device, and a
 * context of gnss_ctx_create_multi. GNSS_EIO: within a window a negative pos_bytes, one that is
 * lower than the row's before, or a difference to the window's first row that is no multiple of
 * bytes_per_sample or exceeds 2^50 bytes. */
int gnss_replay_ddm(gnss_ctx *ctx, const gnss_replay_ddm_cfg *cfg, const gnss_replay_ddm_in *in,
                    gnss_replay_ddm_out *out);

/* ---- multi-ray fit of an ACF on any tap grid (additive within ABI v14; detected by symbol) ----
 * gnss_acf_fit_taps fits one reflected path on an exhaustive (p, e) grid, which cannot grow to a
 * third path. This fit adds paths one at a time by alternating projection (the family MEDLL
 * belongs to): a path's position is searched on a 1-D grid while the others stay fixed, and the
 * amplitudes of all paths are solved jointly for every candidate. Up to GNSS_ACF_MULTI_MAX_PATHS
 * paths, the direct one included. The input is gnss_acf_fit_taps' (gnss_acf_fit_taps_in plus u and
 * prompt), so replayed sums and the 25-tap records go in alike. All arithmetic is fp64, every
 * operation rounded on its own, every sum over all n_taps taps left to right from its first term;
 * csrc/acf_fit_multi.h is the one source for host and device and fixes the order of every
 * operation of step 3.
 *  1. Windows, the rows' signs, the coherent vector z = zI + j zQ and energy = sum_j |z_j|^2 are
 *     exactly gnss_acf_fit_taps'. A non-finite z gives paths = 0, searches = 0 and every floating
 *     output of the window NaN.
 *  2. Candidate positions q_i = q_min + i*q_step, i < q_count, with r_i[j] = R(u[j] - q_i),
 *     R(x) = max(0, 1 - |x|), in orient = +1's convention: a path that arrives later sits at a
 *     lower q. A candidate is usable iff sum_j r_i[j]^2 != 0.
 *  3. The joint fit of an ordered set of m positions (slots 1..m, m <= 4): G_kl = sum_j
 *     r_k[j]*r_l[j], h_k = sum_j r_k[j]*z[j] (I and Q apart); Gaussian elimination without pivoting
 *     in slot order (f = G_ik / d_k; G_il = G_il - f*G_kl for l > k; h_i = h_i - f*h_k), then
 *     back-substitution (s = h_k; s = s - G_kl*A_l for l = k+1..m ascending; A_k = s / d_k). The
 *     set is singular when a pivot fails d_k > (1e-9*G_kk), G_kk the original diagonal. res =
 *     sum_j |((z_j - A_1 r_1j) - A_2 r_2j) - ...|^2. For m = 1 these are the operations of
 *     gnss_acf_fit_taps' one-path hypothesis (A = h/a).
 *  4. Search(k): the other slots fixed, every candidate i is tried in slot k's place, the slot order
 *     kept. Skipped: an unusable i, an i with |i - i_l| < sep_min for another slot l, a singular
 *     set. The lexicographic minimum of (res, i) wins and slot k moves there; a NaN never wins. If
 *     nothing survives the slot stays; when that happens to a slot being appended, that order is
 *     not formed and the orders end there. In a sweep the slot's present position is itself a
 *     survivor, so a sweep never raises res beyond rounding.
 *  5. Orders m = 1..max_paths: slot m is appended with Search(m); then up to `sweeps` rounds, each
 *     Search(1) .. Search(m) in order, a round that moved no slot ending the rounds. The order keeps
 *     its positions and res_m, the last winner's residual; res_0 = energy. `searches` counts the
 *     Search calls of the window: it pins the path taken, not only where it ends.
 *  6. paths = the largest formed m with res_{m-1} > gain_min*res_m (the last significant drop: with
 *     two rays an intermediate order may explain little, and a sequential test would stop there);
 *     1 if no m passes but order 1 was formed; 0 if order 1 was not formed (then q, A and bias are
 *     NaN; res[0] and energy are given).
 *  7. Outputs per window: paths; the selected order's paths by descending q (earliest arrival
 *     first) with the joint amplitudes formed again from its positions: q[k], A_re[k], A_im[k] for
 *     k < paths, NaN beyond; bias = q[0]; res[0..4], every order formed, NaN otherwise; energy;
 *     searches; optionally zI / zQ, which equal gnss_acf_fit_taps' bit for bit. */
#define GNSS_ACF_MULTI_MAX_PATHS 4

typedef struct gnss_acf_fit_multi_cfg {
    int32_t       n;            /* channels, 1..GNSS_VT_MAX_CH                                  */
    int32_t       ind_start;    /* as gnss_acf_cfg, >= 1; default 1                             */
    int32_t       numOverLap;   /* rows per window, 2..4096; default 100                        */
    int32_t       n_taps;       /* 1..GNSS_REPLAY_MAX_TAPS                                      */
    int32_t       prompt;       /* 0..n_taps-1                                                  */
    int32_t       flags;        /* GNSS_OUT_DEVICE: in->taps is a DEVICE pointer, or 0          */
    const double *u;            /* [n_taps] tap coordinates in chips, host, finite              */
    double        q_min, q_step;      /* default -2.40, 0.01; q_step > 0                        */
    int32_t       q_count;      /* 1..4096; default 281 (-2.4..0.4: what -2.5:0.05:1.0 carries) */
    int32_t       max_paths;    /* 1..GNSS_ACF_MULTI_MAX_PATHS; default 3                       */
    int32_t       sweeps;       /* 0..16; default 4; 0 is the plain greedy order                */
    int32_t       sep_min;      /* 1..q_count; default 5                                        */
    double        gain_min;     /* >= 0; default 16.0, the existing fits' value                 */
} gnss_acf_fit_multi_cfg;

typedef struct gnss_acf_fit_multi_out {
    int64_t  cap;               /* windows per channel the arrays hold                          */
    int64_t *windows;           /* [n] windows written per channel                              */
    int32_t *paths;             /* [n][cap]                                                     */
    int32_t *searches;          /* [n][cap]                                                     */
    double  *bias;              /* [n][cap]                                                     */
    double  *q, *A_re, *A_im;   /* [n][4][cap], whatever max_paths is                           */
    double  *res;               /* [n][5][cap]                                                  */
    double  *energy;            /* [n][cap]                                                     */
    double  *zI, *zQ;           /* optional (NULL: not wanted) [n][n_taps][cap]                 */
} gnss_acf_fit_multi_out;

/* The fit over the sums `in`. Host sums need no GPU and ctx may be NULL (up to 16 threads, a window
 * by one thread: the bits do not depend on the thread count); with GNSS_OUT_DEVICE the fit runs on
 * the GPU (csrc/acf_fit_multi.hip, one block per window) and gnss_last_timing's track_kernel_ms
 * holds the kernel's duration. Both paths give the same bits in every output. Everything is checked
 * on the host before any launch; each refusal sets the error text and leaves the outputs untouched
 * and the context usable. GNSS_EARG for a null argument, n, n_taps or prompt out of range, a
 * non-finite u[j], numOverLap outside 2..4096, ind_start < 1, a q_step that is not positive and
 * finite, a non-finite q_min, q_count outside 1..4096, max_paths outside 1..4, sweeps outside 0..16,
 * sep_min outside 1..q_count, a gain_min that is negative or NaN, max_rows < 1, n_rows[c] outside
 * 0..max_rows, more windows than cap, an unknown flag, GNSS_OUT_DEVICE without a context or with
 * taps that is not device memory of the context's device, and device sums on a context of
 * gnss_ctx_create_multi. */
int gnss_acf_fit_multi(gnss_ctx *ctx, const gnss_acf_fit_multi_cfg *cfg,
                       const gnss_acf_fit_taps_in *in, gnss_acf_fit_multi_out *out);

/* The fit alone on one coherent vector zI[n_taps], zQ[n_taps], host only: cfg's n_taps, u, grid and
 * search parameters are read (n, ind_start, numOverLap, prompt beyond its range check and flags are
 * not); out with cap >= 1 gets window 0 of channel 0, zI / zQ, if given, the vector at [j * cap]. */
int gnss_acf_fit_multi_window(const gnss_acf_fit_multi_cfg *cfg, const double *zI, const double *zQ,
                              gnss_acf_fit_multi_out *out);

/* generateCAcode.m:16-64: the 1023 +-1 chips of PRN 1..51 used by the kernels. */
int gnss_ca_code(int prn, int8_t *out1023);

/* ---- synthetic IF: deterministic int8 I/Q record ------------ */
typedef struct gnss_synth_sv {
    int32_t prn;
    double  doppler_hz;     /* carrier Doppler; code Doppler = fd/1575.42e6      */
    double  code_phase0;    /* chips at absolute sample 0 (unwrapped)            */
    double  carr_phase0;    /* cycles at absolute sample 0                       */
    double  cn0_dbhz;
    uint64_t bit_seed;      /* 50 bps nav-bit stream seed                        */
    double  bit_phase_chips;/* nav-bit edge offset, chips                        */
    int32_t lnav;           /* 1: the bits are the LNAV message of gnss_lnav_bits
                               (bit k of the record = bit k mod 3000) instead of
                               seeded random bits; device generator only          */
    int32_t reserved;
} gnss_synth_sv;

typedef struct gnss_synth {
    double   Fs, IF;
    double   noise_sigma;   /* per I/Q component, LSB                            */
    uint64_t seed;
    int32_t  n_sv;
    gnss_synth_sv sv[GNSS_MAX_SV];
} gnss_synth;

/* The synthetic LNAV message (subframes 1-5, TLM/HOW/parity per IS-GPS-200, the
 * ephemeris fields naviDecode_updated.m reads; csrc/lnav.cpp): nbits transmitted bits
 * (0/1) from the start of a subframe 1 with HOW TOW count 65020. */
int gnss_lnav_bits(int32_t prn, int32_t nbits, int8_t *bits_out);

/* Fill dev_dst (this ctx's HBM) with samples [sample0, sample0 + nsamples) of
 * the record, 2 bytes per sample (I then Q). */
int gnss_synth_if_device(gnss_ctx *ctx, const gnss_synth *cfg, uint64_t sample0,
                         uint64_t nsamples, void *dev_dst);

/* ---- synthetic IF with reflected rays (multipath / NLOS scenes) ---------- */
/* The record of gnss_synth with, per SV, a gain on its direct signal and any number of reflected
 * rays: the SV's own code and bit stream later in time, on a carrier of its own. Additive within
 * ABI v13 (detected by symbol); gnss_synth and gnss_synth_if_device are as they were.
 *
 * Per absolute sample n and SV s (amp_s, crate_s, frate_s as gnss_synth_if_device forms them, in
 * double on the host):
 *   th = code_phase0 + (double)n * crate_s; chip floor(th) mod 1023; bit from
 *   floor((th + bit_phase_chips) / 20460); ph = carr_phase0 - (double)n * frate_s, less its floor;
 *   term (amp_s * los_gain[s]) * D * ca[chip] * (cos 2 pi ph, sin 2 pi ph).
 * The direct terms are summed first, in SV order, then the rays in array order. Ray r of SV
 * s = ray[r].sv is present for t_on <= n < t_off:
 *   th_r = th - delay_chips (chip and bit from th_r by the same rules);
 *   ph_r = (carr_phase0_s + phase0_cycles) - (double)n * frate_r, frate_r = (IF + fd + fade_hz)/Fs;
 *   amplitude amp_s * gain.
 * Then the noise, rounding and clipping of gnss_synth_if_device. Sample n depends on n only, and
 * a scene without rays whose los_gain are all 1.0 is gnss_synth_if_device's record byte for byte.
 * Simplification: a ray's delay stays constant while its phase turns (a 1 Hz fade is a path
 * length changing by 0.19 m/s, about 6e-4 chip/s, which the model leaves out). */
#define GNSS_MAX_RAYS 128
typedef struct gnss_synth_ray {
    int32_t  sv;            /* index into gnss_synth_scene.sv, 0..n_sv-1                       */
    int32_t  reserved;
    double   delay_chips;   /* excess path, chips (>= 0)                                       */
    double   gain;          /* amplitude relative to the SV's unattenuated direct signal (>= 0)*/
    double   phase0_cycles; /* carrier phase relative to the direct signal at sample 0         */
    double   fade_hz;       /* carrier frequency relative to the direct signal                 */
    uint64_t t_on, t_off;   /* present for t_on <= n < t_off, absolute samples                 */
} gnss_synth_ray;

typedef struct gnss_synth_scene {
    double   Fs, IF;
    double   noise_sigma;
    uint64_t seed;
    int32_t  n_sv;
    gnss_synth_sv sv[GNSS_MAX_SV];
    double   los_gain[GNSS_MAX_SV];  /* 1.0: gnss_synth's signal; 0.0: NLOS (rays only)         */
    int32_t  n_ray;
    gnss_synth_ray ray[GNSS_MAX_RAYS];  /* dealt over the SVs in any way                       */
} gnss_synth_scene;

/* gnss_synth_if_device for a scene (csrc/synth_scene.hip): fills dev_dst, this ctx's HBM (a
 * multi-device context: devices[0]'s), and drops the members' resident copies of those bytes.
 * GNSS_EARG, before any allocation or launch, for n_sv outside 0..GNSS_MAX_SV, n_ray outside
 * 0..GNSS_MAX_RAYS, a PRN outside 1..51, ray.sv outside 0..n_sv-1, a negative or non-finite
 * delay_chips, gain or los_gain, a non-finite phase0_cycles or fade_hz, and t_off < t_on. */
int gnss_synth_scene_device(gnss_ctx *ctx, const gnss_synth_scene *scene, uint64_t sample0,
                            uint64_t nsamples, void *dev_dst);

/* The same bytes into host memory dst (2 * nsamples bytes) on nthreads CPU threads (0: up to 16).
 * No context and no GPU; the arithmetic is the kernel's (csrc/synth_scene.h). */
int gnss_synth_scene_host(const gnss_synth_scene *scene, uint64_t sample0, uint64_t nsamples,
                          void *dst, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* GNSS_MI355X_H */
