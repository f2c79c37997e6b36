// track_geom.h -- the lane span and grid rule of the tracking steps (api_track.cpp:
// tracking_impl and gnss_correlate_step) as plain functions of plain inputs. Host only, no HIP
// include: tests/native/track_geom.cpp calls the engine's own rule on the CPU.
//
// Geometry: SUB x 8 contiguous samples per lane, 256 lanes per block, bpc blocks per channel;
// SUB grows with the step's total work (more per-lane amortisation once the grid fills the chip).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace gnss {
namespace geom {

constexpr int kLaneThreads = 256;  // lanes per block (= kTrkThreads of the kernels)
constexpr int kVpbMax = 16;        // virtual blocks per resident block (= kMaxVpb)

// What the lane span of a call depends on.
struct LaneRule {
    double cps_max;  // the largest code rate of the call in chips per sample, margin included
    int fmt;         // 0: int8 records, 1: int16 I/Q
    int ntaps;
    bool exact_div;  // k/Fs needs the division (TrkParams::exact_div): 8-sample lanes only
};

// a lane's 8*SUB samples may hold at most one chip boundary per tap: 8*SUB*codeFreq/Fs
// < 1 with margin for the DLL's excursions (the kernel flags a violating step)
inline bool sub_ok(const LaneRule& r, int sub)
{
    return 8.0 * sub * r.cps_max < 1.0 && (sub == 1 || !r.exact_div);
}

// The lane span depends on the step length only (not on the channel set or the path),
// so a channel's sums are bit-identical however the channels are sharded. 1-ms steps
// are latency-bound -> the shortest lanes; 10-ms steps: 24-sample lanes, 96 blocks per
// channel at Opensky rates, which loads the CUs evenly at 8 channels per GPU (3 blocks
// per CU; a step lasts as long as its slowest block).
inline int sub_for(const LaneRule& r, int pdi)
{
    int sub = pdi >= 10 ? 3 : 1;
    while (sub > 1 && !sub_ok(r, sub)) sub--;
    if ((r.fmt == 1 || r.ntaps == 25) && sub != 3) sub = 1;  // (int16, 25 taps: 8- and 24-sample lanes)
    return sub;
}

// `own` unless an override asks for a span the rule admits: `probe` (the probe builds'
// GNSS_FORCE_SUB1 / GNSS_FORCE_SUB10: int8 records below 25 taps), then `forced`
// (GNSS_OPT_FORCE_SUB, the test hook that exercises every kernel variant; int16 and 25 taps
// have the 8- and 24-sample forms only). 0: no override; one that sub_ok rejects is ignored.
inline int sub_override(const LaneRule& r, int own, int probe, int forced)
{
    const bool any_span = r.fmt == 0 && r.ntaps != 25;
    int sub = own;
    if (probe >= 1 && probe <= 4 && sub_ok(r, probe) && any_span) sub = probe;
    if (forced >= 1 && forced <= 4 && sub_ok(r, forced) && (any_span || forced == 1 || forced == 3)) sub = forced;
    return sub;
}

// blocks per channel of a pdi-ms step of S samples per ms (numSample within 1 %)
inline int bpc_for(int64_t S, int pdi, int sub)
{
    const double groups = (S * pdi * 1.01 + 64) / 8.0 + 2;
    return (int)std::ceil(groups / ((double)kLaneThreads * sub));
}

// Virtual blocks per resident block (vpb) of the persistent step loop: 0 = one launch per step
// (no_persist, or no form of the loop fits the chip), 1 = every one of the nch x bpc blocks
// resident, v > 1 = each resident block correlates v of the step's blocks in turn (config 5:
// 32 channels x 11 taps) -- the lane geometry and so the bits stay those of bpc blocks.
// occ1() / occv(): resident blocks per CU of the plain and of the virtual-block kernel form
// (occupancy queries; occv() is asked only when the plain form does not fit, 0: no such form).
// forced_vpb (GNSS_OPT_FORCE_VPB, test hook) asks for at least that many.
template <class Occ1, class OccV>
inline int vpb_for(bool no_persist, int nch, int bpc, int cus, int64_t forced_vpb, Occ1 occ1, OccV occv)
{
    if (no_persist) return 0;
    int v0 = 1;
    if (forced_vpb > 0) v0 = (int)std::min<int64_t>(forced_vpb, kVpbMax);
    const int o1 = std::min((int)occ1(), 4);
    if (v0 == 1 && o1 >= 1 && (int64_t)nch * bpc <= (int64_t)o1 * cus) return 1;
    const int ov = std::min((int)occv(), 4);
    if (ov < 1) return 0;
    for (int v = std::max(v0, 2); v <= kVpbMax; v++)
        if ((int64_t)nch * ((bpc + v - 1) / v) <= (int64_t)ov * cus) return v;
    return 0;
}

}  // namespace geom
}  // namespace gnss
