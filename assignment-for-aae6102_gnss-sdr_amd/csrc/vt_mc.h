// vt_mc.h — the 25-tap vector-tracking step (trackingVT_POS_updated_multicorrelator.m:151-470):
// the scalar arithmetic shared by the host half (vt_mc.cpp), the loop (api_vt.cpp) and the
// correlator kernel (vt_mc.hip), compiled with -ffp-contract=off on every side so each
// operation rounds as MATLAB's does. Line cites are of that file unless they name another.
// What differs from the plain loop (vt_prepare / vt_finish in gnss_internal.h): 25 real
// replicas at Spacing = 0.6:-0.05:-0.6 looked up per sample in a table padded by TWO chips each
// side, E / P / L = Spacing(3) / (13) / (23), remChip from the prompt colon of tap 13.
#pragma once

#include "gnss_internal.h"

namespace gnss {

constexpr int kVtMcTaps = GNSS_VT_MC_TAPS;
constexpr int kVtMcSums = 2 * kVtMcTaps;  // I and Q of every tap
constexpr int kVtMcE = 2, kVtMcP = 12, kVtMcL = 22;  // Spacing(3) / (13) / (23), 0-based

// Spacing = 0.6:-0.05:-0.6 (:26) as MATLAB's colon builds it; element j (0-based)
GNSS_HD double vt_mc_spacing(int j)
{
    return colon_elem(colon_make(0.6, -0.05, -0.6), j);
}

// Code = [c(end) c(end-1) repmat(c,1,pdi) c(1) c(2)] indexed Code(ceil(t) + 2) (:104, :256-281):
// the 0-based C/A chip of m = ceil(t). The pad is in the reference's order: m = 0 reads
// c(end-1) and m = -1 reads c(end); m >= 1 walks the repeated code, whose two chips past the end
// are c(1), c(2) again. Any m maps into 0..1022 (the host rejects m outside -1..1023*pdi+2).
GNSS_HD unsigned vt_mc_chip(int m)
{
    return m >= 1 ? (unsigned)(m - 1) % 1023u : (m == 0 ? 1021u : 1022u);
}

// The step's read size and the 25 replica colons (:155, :218, :230-281): numSample with the LAST
// step's code frequency; tap j's colon (0 + Spacing(j) + remChip) : cps : ((n-1)*cps + Spacing(j)
// + remChip) with the new one as its ends (a, c) -- element k is colon_elem of {a, cps, c, n-1}.
// GNSS_EINDEX where MATLAB raises: a colon without exactly n elements (the .* of :301-350) or a
// table index ceil(t) + 2 outside 1..1023*pdi+4 (the colon rises, so its ends bound every one).
struct VtMcPrep {
    int64_t n;
    double a[kVtMcTaps], c[kVtMcTaps];
    int bad;
};
GNSS_HD VtMcPrep vt_mc_prepare(double Fs, double codelength, int pdi, double remChip, double codeFreq_old,
                               double codeFreq_new)
{
    VtMcPrep p{};
    const double ns = ceil((codelength * pdi - remChip) / (codeFreq_old / Fs));
    if (!(ns >= 1) || ns > 1e9) {
        p.bad = GNSS_EINDEX;
        return p;
    }
    p.n = (int64_t)ns;
    const double cps = codeFreq_new / Fs;  // :218
    const double len = 1023.0 * pdi + 4;
    for (int j = 0; j < kVtMcTaps; j++) {
        const double spc = vt_mc_spacing(j);
        const double a = (0 + spc) + remChip;
        const Colon col = colon_make(a, cps, ((double)(p.n - 1) * cps + spc) + remChip);
        if (col.n != p.n - 1) {
            p.bad = GNSS_EINDEX;
            continue;
        }
        p.a[j] = a;
        p.c[j] = col.c;
        const double lo = ceil(colon_elem(col, 0)) + 2, hi = ceil(colon_elem(col, p.n - 1)) + 2;
        if (!(lo >= 1) || !(hi <= len)) p.bad = GNSS_EINDEX;
    }
    return p;
}

// The rest of the step from its 50 sums (:354-391, :462-470): E / P / L are the real sums of taps
// 3 / 13 / 23; remChip from the prompt colon; remCarrPhase, C/N0, PLL, DLL discriminator and the
// record exactly as vt_finish forms them. Advances `c`. bps = bytes per sample.
GNSS_HD int vt_mc_finish(double Fs, double ms, int pdi, int bps, double tau1carr, double tau2carr, gnss_vt_chan* c,
                         const VtMcPrep& p, double codeFreq_new, const double* tap_i, const double* tap_q,
                         gnss_vt_mc_out* o)
{
    const int64_t n = p.n;
    const double cps = codeFreq_new / Fs;
    const Colon col{p.a[kVtMcP], cps, p.c[kVtMcP], n - 1};
    const double remChip = (colon_elem(col, n - 1) + cps) - 1023 * pdi;  // :354
    const double remCarrPhase = vt_rem_carr_phase(c->carrFreq, n, Fs, c->remCarrPhase);  // :355
    for (int j = 0; j < kVtMcTaps; j++) {
        o->tap_i[j] = tap_i[j];
        o->tap_q[j] = tap_q[j];
    }
    o->E_i = tap_i[kVtMcE];
    o->E_q = tap_q[kVtMcE];
    o->P_i = tap_i[kVtMcP];
    o->P_q = tap_q[kVtMcP];
    o->L_i = tap_i[kVtMcL];
    o->L_q = tap_q[kVtMcL];
    // C/N0 (:362-375)
    o->CN0 = 0;
    o->cn0_row = 0;
    c->index_int += 1;
    c->Zk[c->index_int - 1] = o->P_i * o->P_i + o->P_q * o->P_q;
    if (c->index_int % 20 == 0) {
        o->CN0 = cn0_moment(c->Zk, 1 * ms * pdi);
        o->cn0_row = c->snrIndex;
        c->index_int = 0;
        c->snrIndex += 1;
    }
    const VtPll pll = vt_pll(*c, pdi, tau1carr, tau2carr, o->P_i, o->P_q);  // :378-382
    const double E = sqrt(o->E_i * o->E_i + o->E_q * o->E_q);  // :386-388
    const double L = sqrt(o->L_i * o->L_i + o->L_q * o->L_q);
    o->codeError = -0.5 * (E - L) / (E + L);
    o->carrError = pll.carrError;
    o->carrNco = pll.carrNco;
    o->remChip = remChip;
    o->remCarrPhase = remCarrPhase;
    o->codeFreq = codeFreq_new;
    o->carrFreq = pll.carrFreq;
    o->numSample = n;
    const int64_t absS = c->file_ptr + n * bps;  // ftell after the read (:156-169, :470)
    o->absoluteSample = absS;
    o->codedelay = fmod_pos((double)absS / bps, Fs * ms);
    o->status = GNSS_OK;
    c->file_ptr = absS;
    c->remChip = remChip;
    c->remCarrPhase = remCarrPhase;
    c->codeFreq = codeFreq_new;
    c->carrFreq = pll.carrFreq;
    c->oldCarrNco = pll.carrNco;
    c->oldCarrError = pll.carrError;
    return GNSS_OK;
}

// One step of n channels over n x nb blocks (vt_mc.hip): block b of channel ch correlates the
// samples [b*chunk, (b+1)*chunk) of the read (chunk = ceil(ns / nb)) against the 25 replicas into
// part[(ch*nb + b)*50 ..]; the grid's last block adds each channel's partials in block order into
// sums[ch*50 ..] (I of taps 0..24, then Q) and posts `seq` to *done -- vt_step_kernel's hand-off.
// The host has sized and cleared every read (vt_mc_prepare, the window, the file's length); a
// channel with ns = 0 sits the step out.
struct VtMcStepArgs {
    const uint8_t* rec;             // staged record window
    const unsigned* ca_bits;        // [n][32] C/A chips as sign bits (bit set: -1), device memory
    const long long* isum;          // [n][2] int16 records: the read's integer sums of I and Q, else null
    double Fs;
    int fmt;                        // 0 int8 I/Q, 1 int8 real, 2 int16 I/Q (means removed)
    unsigned seq;                   // the step's number
    double* part;                   // [n][nb][50], device memory
    double* sums;                   // [n][50], coherent host memory
    unsigned* done;                 // [1], coherent host memory
    unsigned* ticket;               // [1], device memory, 0 between launches
    int64_t off[GNSS_VT_MAX_CH];    // the read's first byte in the window
    int64_t ns[GNSS_VT_MAX_CH];     // samples read (0: the channel sits the step out)
    double f[GNSS_VT_MAX_CH];       // carrFreq
    double phi0[GNSS_VT_MAX_CH];    // remCarrPhase
    double rfs[GNSS_VT_MAX_CH];     // RN(1/Fs) if k/Fs = div_markstein for k < ns (host-verified), else 0
    double remChip[GNSS_VT_MAX_CH]; // the colons' remChip and step (each block rebuilds the 25
    double cps[GNSS_VT_MAX_CH];     // colons' ends: vt_mc_prepare's arithmetic, the same bits)
};
hipError_t launch_vt_mc_step(const VtMcStepArgs& a, int n, int nb, hipStream_t s);
// int16 records: the exact integer sums of each channel's read into isum[n][2] (zeroed by the
// caller), by integer atomics -- the same value in any order
hipError_t launch_vt_mc_isum(const uint8_t* rec, const int64_t* off, const int64_t* ns, int n, long long* isum,
                             hipStream_t s);
constexpr int kVtMcStepSamples = 8 * kVtStepThreads;  // samples per block at the nominal read

}  // namespace gnss
