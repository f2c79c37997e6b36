"""ctypes mirror of include/gnss_mi355x.h (the C-ABI drop-in boundary).

The struct layouts here must match the header field for field; tests check the
sizes against a tiny compiled probe. The product library is
``lib/libgnss_mi355x.so`` next to this file (built in-tree by
``__graft_entry__.build()``); if it is missing every entry point raises — there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

MAX_SV = 64
MAX_TAPS = 32

OK, ENODATA, EIO, EARG, EDEVICE, EINDEX = 0, 1, 2, 3, 4, 5

FIELDS = ["P_i", "P_q", "E_i", "E_q", "L_i", "L_q", "PLLdiscri", "DLLdiscri", "codedelay",
          "remChip", "codeFreq", "carrierFreq", "remPhase", "remSample", "numSample",
          "delayValue", "absoluteSample", "codedelay2"]
NFIELDS = len(FIELDS)
OUT_DEVICE = 1  # gnss_track_out.flags: rec / taps are device pointers (ABI v7)
# the same slots under trackingCT_POS_updated.m:273-292's names (gnss_tracking_ct_pos)
FIELDS_POS = ["P_i", "P_q", "E_i", "E_q", "L_i", "L_q", "carrError", "codeError", "codedelay",
              "remChip", "codeFreq", "carrFreq", "remCarrPhase", "absoluteSampleCodedelay",
              "numSample", "delayValue", "absoluteSample", "codedelay2"]

# the 25 taps of trackingCT_POS_updated_multicorrelator.m in Spacing order (0.6:-0.05:-0.6,
# :41), under the names of its TckResultCT fields (:374-423)
MC_TAPS = 25
MC_TAP_NAMES = ([f"E_{{}}{s}" for s in ["_060", "_055", "", "_045", "_040", "_035", "_030", "_025",
                                         "_020", "_015", "_010", "_005"]] + ["P_{}"] +
                [f"L_{{}}{s}" for s in ["005", "010", "015", "020", "025", "030", "035", "040", "045",
                                         "", "055", "060"]])


# ephemeris(prn) fields of naviDecode_updated.m (ini_eph.m order; updateflag separate)
EPH_FIELDS = ["TOW", "TOW1", "sfb", "sfb1", "weeknum", "N", "health", "IODC", "TGD", "toc", "af2",
              "af1", "af0", "IODE2", "Crs", "deltan", "M0", "Cuc", "ecc", "Cus", "sqrta", "toe", "Cic",
              "omegae", "Cis", "i0", "Crc", "w", "omegadot", "IODE3", "idot", "updatetime",
              "updatetime_tow"]
EPH_NFIELDS = len(EPH_FIELDS)


class GnssNavOut(C.Structure):
    _fields_ = [("eph_cap", C.c_int32), ("eph", C.POINTER(C.c_double)),
                ("eph_len", C.POINTER(C.c_int32)), ("updateflag", C.POINTER(C.c_int32)),
                ("nav1", C.POINTER(C.c_int64)), ("sfb1", C.POINTER(C.c_int64))]


class GnssFile(C.Structure):
    _fields_ = [("path", C.c_char_p), ("data", C.c_void_p), ("dev_data", C.c_void_p),
                ("nbytes", C.c_uint64), ("skip", C.c_int64), ("dataType", C.c_int32),
                ("dataPrecision", C.c_int32)]


class GnssSignal(C.Structure):
    _fields_ = [("IF", C.c_double), ("Fs", C.c_double), ("codeFreqBasis", C.c_double),
                ("ms", C.c_double), ("Sample", C.c_int64), ("codelength", C.c_double)]


class GnssAcq(C.Structure):
    _fields_ = [("freqNum", C.c_int32), ("freqMin", C.c_double), ("freqStep", C.c_double),
                ("datalen", C.c_int32), ("L", C.c_int32), ("n_prn", C.c_int32),
                ("prn_list", C.POINTER(C.c_int32))]


class GnssAcquired(C.Structure):
    _fields_ = [("n", C.c_int32), ("sv", C.c_int32 * MAX_SV), ("SNR", C.c_double * MAX_SV),
                ("Doppler", C.c_double * MAX_SV), ("codedelay", C.c_int32 * MAX_SV),
                ("fineFreq", C.c_double * MAX_SV)]


class GnssAcqDiag(C.Structure):
    _fields_ = [("n", C.c_int32), ("prn", C.c_int32 * MAX_SV), ("SNR", C.c_double * MAX_SV),
                ("fbin", C.c_int32 * MAX_SV), ("codePhase", C.c_int32 * MAX_SV),
                ("peak", C.c_double * MAX_SV), ("peak2", C.c_double * MAX_SV)]


class GnssTrack(C.Structure):
    _fields_ = [("CorrelatorSpacing", C.c_double), ("DLLBW", C.c_double), ("DLLDamp", C.c_double),
                ("DLLGain", C.c_double), ("PLLBW", C.c_double), ("PLLDamp", C.c_double),
                ("PLLGain", C.c_double), ("msToProcessCT_1ms", C.c_int32),
                ("msToProcessCT_10ms", C.c_int32), ("n_taps", C.c_int32),
                ("tap_offsets", C.POINTER(C.c_double)), ("n_chan", C.c_int32),
                ("chan", C.POINTER(C.c_int32))]


class GnssTrackOut(C.Structure):
    _fields_ = [("max_len", C.c_int64), ("rec", C.POINTER(C.c_double)),
                ("taps", C.POINTER(C.c_double)), ("len", C.POINTER(C.c_int64)),
                ("countinx", C.POINTER(C.c_int32)), ("CN0_Eph", C.POINTER(C.c_double)),
                ("cn0_cap", C.c_int32), ("cn0_rows", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class GnssTiming(C.Structure):
    _fields_ = [("acq_ms", C.c_double), ("acq_corr_ms", C.c_double), ("acq_fine_ms", C.c_double),
                ("track_ms", C.c_double), ("track_kernel_ms", C.c_double),
                ("track_launches", C.c_int64), ("track_channel_samples", C.c_int64),
                ("acq_hypothesis_samples", C.c_int64), ("h2d_ms", C.c_double),
                ("track10_kernel_ms", C.c_double), ("track10_launches", C.c_int64),
                ("track10_channel_samples", C.c_int64), ("h2d_bytes", C.c_int64),
                ("track_segments", C.c_int64)]


class GnssVtChan(C.Structure):
    _fields_ = [("prn", C.c_int32), ("pad", C.c_int32), ("file_ptr", C.c_int64), ("remChip", C.c_double),
                ("remCarrPhase", C.c_double), ("codeFreq", C.c_double), ("carrFreq", C.c_double),
                ("carrFreqBasis", C.c_double), ("oldCarrNco", C.c_double), ("oldCarrError", C.c_double),
                ("index_int", C.c_int32), ("snrIndex", C.c_int32), ("Zk", C.c_double * 20)]


class GnssVtOut(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("E_i", "E_q", "P_i", "P_q", "L_i", "L_q", "carrError", "codeError",
                                          "carrNco", "remChip", "remCarrPhase", "codeFreq", "carrFreq")] + \
               [("numSample", C.c_int64), ("absoluteSample", C.c_int64), ("codedelay", C.c_double),
                ("CN0", C.c_double), ("cn0_row", C.c_int32), ("status", C.c_int32),
                ("deltaPr", C.c_double), ("prRate", C.c_double), ("sv_vel", C.c_double * 3)]


class GnssVtMcOut(C.Structure):
    """gnss_vt_mc_out: gnss_vt_out's fields, then the 25-tap loop's 50 sums in Spacing order
    (trackingVT_POS_updated_multicorrelator.m; additive within ABI v13)."""
    _fields_ = GnssVtOut._fields_ + [("tap_i", C.c_double * MC_TAPS), ("tap_q", C.c_double * MC_TAPS)]


# the structs added within an ABI version: name in include/gnss_mi355x.h -> mirror here (their
# layout is checked like the older ones', tests/test_vt_mc_twin.py)
ADDED_STRUCTS = {"gnss_vt_mc_out": "GnssVtMcOut"}

# the vector half of trackingVT_POS_updated.m (ABI v10)
VT_MAX_CH = 32
EPH_SV_FIELDS = ["sqrta", "deltan", "toe", "M0", "ecc", "w", "Cus", "Cuc", "Crs", "Crc", "Cis", "Cic", "i0",
                 "idot", "omegae", "omegadot", "toc", "af0", "af1", "af2", "TGD"]
GEO_XYZ2LLH, GEO_LLH2XYZ, GEO_XYZ2ENU, GEO_EROTCORR, GEO_IONO, GEO_TROP = range(6)


class GnssEphSv(C.Structure):
    _fields_ = [(f, C.c_double) for f in EPH_SV_FIELDS]


class GnssVtNavCfg(C.Structure):
    _fields_ = [("cnslxyz", C.c_double * 3), ("ALPHA", C.c_double * 4), ("BETA", C.c_double * 4),
                ("doy", C.c_double), ("cSpeed", C.c_double), ("Fc", C.c_double)]


class GnssVtNav(C.Structure):
    _fields_ = [("n", C.c_int32), ("pdi", C.c_int32), ("msIndex", C.c_int32), ("counterUptR", C.c_int32),
                ("counter_r", C.c_int32), ("prn", C.c_int32 * VT_MAX_CH), ("cfg", GnssVtNavCfg),
                ("Fs", C.c_double), ("IF", C.c_double), ("codeFreqBasis", C.c_double), ("ms", C.c_double),
                ("cnslxyz", C.c_double * 3), ("total_state", C.c_double * 8), ("state_cov", C.c_double * 64),
                ("R", C.c_double * (2 * VT_MAX_CH)), ("recordR2", C.c_double * (2 * VT_MAX_CH))] + \
               [(f, C.c_double * VT_MAX_CH) for f in ("transmitTime", "tot_est_tck", "predictedPr_last",
                                                     "counter_corr", "ionodel", "tropodel", "el", "az")] + \
               [("numSample", C.c_int64 * VT_MAX_CH), ("eph", GnssEphSv * VT_MAX_CH)]


class GnssVtNavSol(C.Structure):
    _fields_ = [("localTime", C.c_double)] + \
               [(f, C.c_double * 3) for f in ("usrPos", "usrVel", "usrPosENU", "usrVelENU", "usrPosLLH")] + \
               [("clkBias", C.c_double), ("clkDrift", C.c_double), ("state", C.c_double * 8),
                ("state_cov", C.c_double * 8), ("newZ", C.c_double * (2 * VT_MAX_CH)),
                ("meas_inno", C.c_double * (2 * VT_MAX_CH)), ("satEA", C.c_double * VT_MAX_CH),
                ("satAZ", C.c_double * VT_MAX_CH), ("predicted_z", C.c_double * (2 * VT_MAX_CH)),
                ("satePos", C.c_double * 3), ("sateVel", C.c_double * 3),
                ("svxyz_pos", (C.c_double * 3) * VT_MAX_CH), ("kalman_gain", (C.c_double * (2 * VT_MAX_CH)) * 8),
                ("R", C.c_double * (2 * VT_MAX_CH)), ("r_row", C.c_int32),
                ("reserved", C.c_int32)]


# the positioning half of trackingCT_POS_updated.m (gnss_ct_pos_solve; additive within ABI v13)
ENOCONV = 6
CT_POS_UPDATED, CT_POS_MULTICORR = 0, 1
# navSolutionsCT's fields (trackingCT_POS_updated.m:509-551) and their values per row (0: n)
NAVSOL_CT_FIELDS = [("rawPseudorange", 0), ("usrPos", 3), ("usrVel", 3), ("usrPosENU", 3), ("usrPosLLH", 3),
                    ("clkBias", 1), ("usrVelENU", 3), ("clkDrift", 1), ("DOP", 4), ("satEA", 0), ("satAZ", 0),
                    ("timeTransmit", 0), ("codePhaseMeas", 0), ("localTime", 1)]


class GnssCtPosCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("mode", C.c_int32), ("dataType", C.c_int32), ("msToProcessCT_1ms", C.c_int32),
                ("pdi", C.c_int32), ("reserved", C.c_int32), ("navSolPeriod", C.c_double), ("Fs", C.c_double),
                ("IF", C.c_double), ("codelength", C.c_double), ("ms", C.c_double), ("cSpeed", C.c_double),
                ("doy", C.c_double), ("cnslxyz", C.c_double * 3), ("ALPHA", C.c_double * 4),
                ("BETA", C.c_double * 4), ("countinx", C.c_int32 * VT_MAX_CH), ("nav1", C.c_int64 * VT_MAX_CH),
                ("sfb1", C.c_int64 * VT_MAX_CH), ("sampleStart", C.c_int64 * VT_MAX_CH),
                ("TOW1", C.c_double * VT_MAX_CH), ("eph", GnssEphSv * VT_MAX_CH)]


class GnssNavSolCt(C.Structure):
    _fields_ = [("cap", C.c_int64), ("rows", C.c_int64)] + \
               [(f, C.POINTER(C.c_double)) for f, _ in NAVSOL_CT_FIELDS] + \
               [("Index", C.POINTER(C.c_int64)), ("index", C.POINTER(C.c_int64)),
                ("carrFreqMeas", C.POINTER(C.c_double)), ("iters", C.POINTER(C.c_int32))]


ADDED_STRUCTS.update({"gnss_ct_pos_cfg": "GnssCtPosCfg", "gnss_nav_sol_ct": "GnssNavSolCt"})

# ACF/CalculateFeatures.m (gnss_acf_features; additive within ABI v13): the script's parameters
# (:172-179, :186) and the per-window outputs in data_labeled's column order (:277-282)
ACF_DEFAULTS = dict(ind_start=1, numOverLap=100, corrSpacing=0.05, maxDelay=0.6,
                    a=(4092.9779845217, 340.423503277404, -2.99026922880033, 0.0251763660254827))
ACF_FIELDS = ["meanMax", "F1", "F2", "varDelay", "meanCodeDisc", "varCodeDisc"]


class GnssAcfCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("ind_start", C.c_int32), ("numOverLap", C.c_int32), ("reserved", C.c_int32),
                ("corrSpacing", C.c_double), ("maxDelay", C.c_double), ("a", C.c_double * 4),
                ("prn", C.c_int32 * VT_MAX_CH), ("ele", C.c_double * VT_MAX_CH)]


class GnssAcfOut(C.Structure):
    _fields_ = [("cap", C.c_int64), ("windows", C.POINTER(C.c_int64))] + \
               [(f, C.POINTER(C.c_double)) for f in ACF_FIELDS] + \
               [("maxCorrInd", C.c_void_p), ("corr", C.c_void_p)]


ADDED_STRUCTS.update({"gnss_acf_cfg": "GnssAcfCfg", "gnss_acf_out": "GnssAcfOut"})

# The script's F6-F8 (gnss_acf_features_ext; additive within ABI v13): the history's length (:231),
# the spectrum's (:264) and the departure on offer; fs has no default here, it follows from
# numOverLap and pdi (:172). The outputs in the 11-column data_labeled's order (:32).
ACF_EXT_DEFAULTS = dict(fft_hist=300, fft_n=1024, fft_fill=0)
ACF_EXT_FIELDS = ("numMLC", "fftFreq", "fftMag")


class GnssAcfExtCfg(C.Structure):
    _fields_ = [("fft_hist", C.c_int32), ("fft_n", C.c_int32), ("fft_fill", C.c_int32), ("reserved", C.c_int32),
                ("fs", C.c_double)]


class GnssAcfExtOut(C.Structure):
    _fields_ = [(f, C.POINTER(C.c_double)) for f in ACF_EXT_FIELDS]


ADDED_STRUCTS.update({"gnss_acf_ext_cfg": "GnssAcfExtCfg", "gnss_acf_ext_out": "GnssAcfExtOut"})

# The two-path fit of the 25-tap ACF (gnss_acf_fit / gnss_acf_fit_window; additive within ABI
# v13): the windows' parameters as above, the grid and the two thresholds; `orient` has no
# default (the 25-tap loops' wrappers tag their results with it: ACF_ORIENT)
ACF_FIT_DEFAULTS = dict(ind_start=1, numOverLap=100, corrSpacing=0.05, p_min=-0.40, p_step=0.01, p_count=81,
                        e_min=0.05, e_step=0.01, e_count=96, ratio_max=1.0, gain_min=16.0)
ACF_FIT_FIELDS = ["bias", "p1", "A1p_re", "A1p_im", "res1", "p0", "e", "A0_re", "A0_im", "A1_re", "A1_im", "res2",
                  "energy"]
# u[j] = orient * (j - 12) * corrSpacing is the loop's Spacing(j): -0.6:0.05:0.6 in
# trackingCT_multiCorr-GIVEN.m:25, 0.6:-0.05:-0.6 in the two _multicorrelator loops
ACF_ORIENT = dict(trackingCT_multiCorr=1, trackingCT_POS_updated_multicorrelator=-1,
                  trackingVT_POS_updated_multicorrelator=-1)


class GnssAcfFitCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("ind_start", C.c_int32), ("numOverLap", C.c_int32), ("orient", C.c_int32),
                ("corrSpacing", C.c_double), ("p_min", C.c_double), ("p_step", C.c_double), ("e_min", C.c_double),
                ("e_step", C.c_double), ("p_count", C.c_int32), ("e_count", C.c_int32), ("ratio_max", C.c_double),
                ("gain_min", C.c_double)]


class GnssAcfFitOut(C.Structure):
    _fields_ = [("cap", C.c_int64), ("windows", C.POINTER(C.c_int64)), ("paths", C.POINTER(C.c_int32))] + \
               [(f, C.POINTER(C.c_double)) for f in ACF_FIT_FIELDS] + \
               [("zI", C.POINTER(C.c_double)), ("zQ", C.POINTER(C.c_double))]


ADDED_STRUCTS.update({"gnss_acf_fit_cfg": "GnssAcfFitCfg", "gnss_acf_fit_out": "GnssAcfFitOut"})

# The k-NN classifier over the feature windows (gnss_knn_standardize / gnss_knn_classify; additive
# within ABI v13): its limits and the two flags
KNN_MAX_D, KNN_MAX_K, KNN_MAX_CLASS, KNN_MAX_M = 16, 32, 8, 1 << 24
KNN_HOST = 1          # gnss_knn_cfg.flags
KNN_MODEL_DEVICE = 1  # gnss_knn_model.flags


class GnssKnnCfg(C.Structure):
    _fields_ = [("k", C.c_int32), ("flags", C.c_int32)]


class GnssKnnModel(C.Structure):
    _fields_ = [("M", C.c_int64), ("D", C.c_int32), ("n_class", C.c_int32), ("mu", C.c_void_p), ("inv", C.c_void_p),
                ("z", C.c_void_p), ("label", C.c_void_p), ("flags", C.c_int32), ("reserved", C.c_int32)]


class GnssKnnOut(C.Structure):
    _fields_ = [("label", C.c_void_p), ("votes", C.c_void_p), ("nn_index", C.c_void_p), ("nn_d2", C.c_void_p)]


ADDED_STRUCTS.update({"gnss_knn_cfg": "GnssKnnCfg", "gnss_knn_model": "GnssKnnModel", "gnss_knn_out": "GnssKnnOut"})

# The replay correlator (gnss_replay_correlate; additive within ABI v13): recorded tracking rows
# correlated again on any tap grid
REPLAY_MAX_TAPS = 256


class GnssReplayCfg(C.Structure):
    _fields_ = [("n_taps", C.c_int32), ("chip_off", C.c_int32), ("tap_offsets", C.c_void_p), ("post", C.c_void_p),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class GnssReplayRows(C.Structure):
    _fields_ = [("n_chan", C.c_int32), ("reserved", C.c_int32), ("max_rows", C.c_int64), ("prn", C.c_void_p),
                ("n_rows", C.c_void_p), ("pos_bytes", C.c_void_p), ("numSample", C.c_void_p), ("remChip", C.c_void_p),
                ("codeFreq", C.c_void_p), ("carrFreq", C.c_void_p), ("remPhase", C.c_void_p)]


class GnssReplayOut(C.Structure):
    _fields_ = [("taps", C.c_void_p), ("kernel_ms", C.c_double)]


ADDED_STRUCTS.update({"gnss_replay_cfg": "GnssReplayCfg", "gnss_replay_rows": "GnssReplayRows",
                      "gnss_replay_out": "GnssReplayOut"})

# The two-path fit on any tap grid (gnss_acf_fit_taps / gnss_acf_fit_taps_window; additive within
# ABI v13): gnss_acf_fit's grid with e up to 2.00 chips, for the wider grids of a replay; the taps'
# coordinates u and the prompt's index come with the call
ACF_FIT_TAPS_DEFAULTS = dict(ind_start=1, numOverLap=100, p_min=-0.40, p_step=0.01, p_count=81, e_min=0.05,
                             e_step=0.01, e_count=196, ratio_max=1.0, gain_min=16.0)


class GnssAcfFitTapsCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("ind_start", C.c_int32), ("numOverLap", C.c_int32), ("n_taps", C.c_int32),
                ("prompt", C.c_int32), ("flags", C.c_int32), ("u", C.c_void_p), ("p_min", C.c_double),
                ("p_step", C.c_double), ("e_min", C.c_double), ("e_step", C.c_double), ("p_count", C.c_int32),
                ("e_count", C.c_int32), ("ratio_max", C.c_double), ("gain_min", C.c_double)]


class GnssAcfFitTapsIn(C.Structure):
    _fields_ = [("taps", C.c_void_p), ("max_rows", C.c_int64), ("n_rows", C.c_void_p)]


ADDED_STRUCTS.update({"gnss_acf_fit_taps_cfg": "GnssAcfFitTapsCfg", "gnss_acf_fit_taps_in": "GnssAcfFitTapsIn"})

# The delay-Doppler map over replayed rows (gnss_replay_ddm; additive within ABI v14): a window's
# rows summed coherently with one rotation per row, per (tap, Doppler offset) cell, and its peaks
DDM_MAX_DOPP = 256
DDM_MAP_DEVICE = 2  # with OUT_DEVICE: out.map is device memory and stays there


class GnssReplayDdmCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_taps", C.c_int32), ("prompt", C.c_int32), ("rows_per_window", C.c_int32),
                ("n_dopp", C.c_int32), ("flags", C.c_int32), ("dopp_hz", C.c_void_p), ("u", C.c_void_p),
                ("excl_chips", C.c_double), ("excl_hz", C.c_double), ("Fs", C.c_double),
                ("bytes_per_sample", C.c_int32), ("reserved", C.c_int32)]


class GnssReplayDdmIn(C.Structure):
    _fields_ = [("taps", C.c_void_p), ("max_rows", C.c_int64), ("n_rows", C.c_void_p), ("pos_bytes", C.c_void_p),
                ("numSample", C.c_void_p)]


class GnssReplayDdmOut(C.Structure):
    _fields_ = [("cap", C.c_int64), ("map", C.c_void_p), ("peak_bin", C.c_void_p), ("peak_tap", C.c_void_p),
                ("peak_pow", C.c_void_p), ("sec_bin", C.c_void_p), ("sec_tap", C.c_void_p), ("sec_pow", C.c_void_p),
                ("n_win", C.c_void_p), ("kernel_ms", C.c_double)]


ADDED_STRUCTS.update({"gnss_replay_ddm_cfg": "GnssReplayDdmCfg", "gnss_replay_ddm_in": "GnssReplayDdmIn",
                      "gnss_replay_ddm_out": "GnssReplayDdmOut"})

# The multi-ray fit on any tap grid (gnss_acf_fit_multi / gnss_acf_fit_multi_window; additive within
# ABI v14): up to ACF_MULTI_MAX_PATHS paths by alternating projection on the candidate grid q; the
# input is gnss_acf_fit_taps' (GnssAcfFitTapsIn, u, prompt). q_min..: -2.4..0.4, what the replay grid
# -2.5:0.05:1.0 can carry
ACF_MULTI_MAX_PATHS = 4
ACF_FIT_MULTI_DEFAULTS = dict(ind_start=1, numOverLap=100, q_min=-2.40, q_step=0.01, q_count=281, max_paths=3,
                              sweeps=4, sep_min=5, gain_min=16.0)


class GnssAcfFitMultiCfg(C.Structure):
    _fields_ = [("n", C.c_int32), ("ind_start", C.c_int32), ("numOverLap", C.c_int32), ("n_taps", C.c_int32),
                ("prompt", C.c_int32), ("flags", C.c_int32), ("u", C.c_void_p), ("q_min", C.c_double),
                ("q_step", C.c_double), ("q_count", C.c_int32), ("max_paths", C.c_int32), ("sweeps", C.c_int32),
                ("sep_min", C.c_int32), ("gain_min", C.c_double)]


class GnssAcfFitMultiOut(C.Structure):
    _fields_ = [("cap", C.c_int64), ("windows", C.POINTER(C.c_int64)), ("paths", C.POINTER(C.c_int32)),
                ("searches", C.POINTER(C.c_int32))] + \
               [(f, C.POINTER(C.c_double)) for f in ("bias", "q", "A_re", "A_im", "res", "energy", "zI", "zQ")]


ADDED_STRUCTS.update({"gnss_acf_fit_multi_cfg": "GnssAcfFitMultiCfg", "gnss_acf_fit_multi_out": "GnssAcfFitMultiOut"})


class GnssSynthSv(C.Structure):
    _fields_ = [("prn", C.c_int32), ("doppler_hz", C.c_double), ("code_phase0", C.c_double),
                ("carr_phase0", C.c_double), ("cn0_dbhz", C.c_double), ("bit_seed", C.c_uint64),
                ("bit_phase_chips", C.c_double), ("lnav", C.c_int32), ("reserved", C.c_int32)]


class GnssSynth(C.Structure):
    _fields_ = [("Fs", C.c_double), ("IF", C.c_double), ("noise_sigma", C.c_double),
                ("seed", C.c_uint64), ("n_sv", C.c_int32), ("sv", GnssSynthSv * MAX_SV)]


# Multipath / NLOS scenes (gnss_synth_scene_device / _host; additive within ABI v13): gnss_synth's
# fields, a gain per SV on its direct signal and the reflected rays
MAX_RAYS = 128


class GnssSynthRay(C.Structure):
    _fields_ = [("sv", C.c_int32), ("reserved", C.c_int32), ("delay_chips", C.c_double), ("gain", C.c_double),
                ("phase0_cycles", C.c_double), ("fade_hz", C.c_double), ("t_on", C.c_uint64),
                ("t_off", C.c_uint64)]


class GnssSynthScene(C.Structure):
    _fields_ = [("Fs", C.c_double), ("IF", C.c_double), ("noise_sigma", C.c_double),
                ("seed", C.c_uint64), ("n_sv", C.c_int32), ("sv", GnssSynthSv * MAX_SV),
                ("los_gain", C.c_double * MAX_SV), ("n_ray", C.c_int32), ("ray", GnssSynthRay * MAX_RAYS)]


ADDED_STRUCTS.update({"gnss_synth_ray": "GnssSynthRay", "gnss_synth_scene": "GnssSynthScene"})


# exported symbols and their prototypes (checked by tests against the header)
PROTOTYPES = {
    "gnss_abi_version": (C.c_int, []),
    "gnss_strerror": (C.c_char_p, [C.c_int]),
    "gnss_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "gnss_ctx_create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "gnss_ctx_members": (C.c_int, [C.c_void_p]),
    "gnss_ctx_drop_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gnss_ctx_resident_records": (C.c_int, [C.c_void_p]),
    "gnss_device_count": (C.c_int, []),
    "gnss_ctx_destroy": (None, [C.c_void_p]),
    "gnss_last_error": (C.c_char_p, [C.c_void_p]),
    "gnss_last_timing": (C.c_int, [C.c_void_p, C.POINTER(GnssTiming)]),
    "gnss_ctx_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "gnss_ctx_set_acq_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "gnss_ctx_set_window": (C.c_int, [C.c_void_p, C.c_uint64]),
    "gnss_ctx_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "gnss_dev_alloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "gnss_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gnss_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gnss_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gnss_acquisition": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                   C.POINTER(GnssAcq), C.POINTER(GnssAcquired),
                                   C.POINTER(GnssAcqDiag)]),
    "gnss_acquisition_surface": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                           C.POINTER(GnssAcq), C.POINTER(C.c_double),
                                           C.POINTER(GnssAcqDiag)]),
    "gnss_tracking_ct": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                   C.POINTER(GnssTrack), C.POINTER(GnssAcquired),
                                   C.POINTER(GnssTrackOut)]),
    "gnss_tracking_ct_pos": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                       C.POINTER(GnssTrack), C.POINTER(GnssAcquired), C.c_int32,
                                       C.POINTER(C.c_int32), C.POINTER(GnssTrackOut)]),
    "gnss_tracking_ct_mc": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                      C.POINTER(GnssTrack), C.POINTER(GnssAcquired), C.c_int32,
                                      C.c_int32, C.POINTER(GnssTrackOut)]),
    "gnss_tracking_ct_multicorr": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                             C.POINTER(GnssTrack), C.POINTER(GnssAcquired), C.c_int32,
                                             C.POINTER(GnssTrackOut)]),
    "gnss_navi_decode": (C.c_int, [C.POINTER(GnssAcquired), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64), C.c_int64, C.POINTER(GnssNavOut)]),
    "gnss_lnav_bits": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "gnss_ca_code": (C.c_int, [C.c_int, C.c_void_p]),
    "gnss_correlate_step": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                      C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "gnss_synth_if_device": (C.c_int, [C.c_void_p, C.POINTER(GnssSynth), C.c_uint64, C.c_uint64,
                                       C.c_void_p]),
    "gnss_synth_scene_device": (C.c_int, [C.c_void_p, C.POINTER(GnssSynthScene), C.c_uint64, C.c_uint64,
                                          C.c_void_p]),
    "gnss_synth_scene_host": (C.c_int, [C.POINTER(GnssSynthScene), C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]),
    "gnss_tracking_vt_run": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                       C.POINTER(GnssTrack), C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(GnssVtChan), C.POINTER(C.c_double), C.POINTER(GnssVtOut)]),
    "gnss_tracking_vt_step": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                        C.POINTER(GnssTrack), C.c_int32, C.c_int32, C.POINTER(GnssVtChan),
                                        C.POINTER(C.c_double), C.POINTER(GnssVtOut)]),
    "gnss_vt_nco_step": (C.c_int, [C.POINTER(GnssSignal), C.POINTER(GnssTrack), C.c_int32,
                                   C.POINTER(GnssVtChan), C.c_double, C.c_double, C.c_double,
                                   C.POINTER(GnssVtOut)]),
    "gnss_vt_prepare": (C.c_int, [C.POINTER(GnssSignal), C.c_int32, C.POINTER(GnssVtChan), C.c_double,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "gnss_sv_pos_vel": (C.c_int, [C.POINTER(GnssEphSv), C.c_double, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
    "gnss_geo": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gnss_vt_nav_init": (C.c_int, [C.POINTER(GnssVtNavCfg), C.POINTER(GnssSignal), C.c_int32, C.c_int32,
                                   C.POINTER(C.c_int32), C.POINTER(GnssEphSv), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_double),
                                   C.POINTER(GnssVtNav)]),
    "gnss_vt_nav_predict": (C.c_int, [C.POINTER(GnssVtNav), C.c_int32, C.c_int64, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gnss_vt_nav_update": (C.c_int, [C.POINTER(GnssVtNav), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(GnssVtNavSol)]),
    "gnss_tracking_vt": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal), C.POINTER(GnssTrack),
                                   C.c_int32, C.c_int32, C.POINTER(GnssVtChan), C.POINTER(GnssVtNav),
                                   C.POINTER(GnssVtOut), C.POINTER(GnssVtNavSol)]),
    # trackingVT_POS_updated_multicorrelator.m (additive within ABI v13: detected by symbol)
    "gnss_tracking_vt_mc_run": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                          C.POINTER(GnssTrack), C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(GnssVtChan), C.POINTER(C.c_double), C.POINTER(GnssVtMcOut)]),
    "gnss_tracking_vt_mc": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal), C.POINTER(GnssTrack),
                                      C.c_int32, C.c_int32, C.POINTER(GnssVtChan), C.POINTER(GnssVtNav),
                                      C.POINTER(GnssVtMcOut), C.POINTER(GnssVtNavSol)]),
    "gnss_vt_mc_prepare": (C.c_int, [C.POINTER(GnssSignal), C.c_int32, C.POINTER(GnssVtChan), C.c_double,
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "gnss_vt_mc_nco_step": (C.c_int, [C.POINTER(GnssSignal), C.POINTER(GnssTrack), C.c_int32,
                                      C.POINTER(GnssVtChan), C.c_double, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(GnssVtMcOut)]),
    "gnss_vt_mc_nav_update": (C.c_int, [C.POINTER(GnssVtNav), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(GnssVtNavSol)]),
    # trackingCT_POS_updated.m's positioning half (additive within ABI v13: detected by symbol)
    "gnss_ct_pos_solve": (C.c_int, [C.c_void_p, C.POINTER(GnssCtPosCfg), C.POINTER(GnssTrackOut),
                                    C.POINTER(GnssNavSolCt)]),
    # ACF/CalculateFeatures.m over the 25-tap records (additive within ABI v13: detected by symbol)
    "gnss_acf_features": (C.c_int, [C.c_void_p, C.POINTER(GnssAcfCfg), C.POINTER(GnssTrackOut), C.c_int32,
                                    C.POINTER(GnssAcfOut)]),
    "gnss_acf_features_ext": (C.c_int, [C.c_void_p, C.POINTER(GnssAcfCfg), C.POINTER(GnssAcfExtCfg),
                                        C.POINTER(GnssTrackOut), C.c_int32, C.POINTER(GnssAcfOut),
                                        C.POINTER(GnssAcfExtOut)]),
    "gnss_acf_twiddle": (C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # the two-path fit of the 25-tap ACF (additive within ABI v13: detected by symbol)
    "gnss_acf_fit": (C.c_int, [C.c_void_p, C.POINTER(GnssAcfFitCfg), C.POINTER(GnssTrackOut), C.c_int32,
                               C.POINTER(GnssAcfFitOut)]),
    "gnss_acf_fit_window": (C.c_int, [C.POINTER(GnssAcfFitCfg), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(GnssAcfFitOut)]),
    # the k-NN classifier over the feature windows (additive within ABI v13: detected by symbol)
    "gnss_knn_standardize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnss_knn_classify": (C.c_int, [C.c_void_p, C.POINTER(GnssKnnCfg), C.POINTER(GnssKnnModel), C.c_void_p,
                                    C.c_int64, C.POINTER(GnssKnnOut)]),
    # the replay correlator (additive within ABI v13: detected by symbol)
    "gnss_replay_correlate": (C.c_int, [C.c_void_p, C.POINTER(GnssFile), C.POINTER(GnssSignal),
                                        C.POINTER(GnssReplayCfg), C.POINTER(GnssReplayRows),
                                        C.POINTER(GnssReplayOut)]),
    # the two-path fit on any tap grid (additive within ABI v13: detected by symbol)
    "gnss_acf_fit_taps": (C.c_int, [C.c_void_p, C.POINTER(GnssAcfFitTapsCfg), C.POINTER(GnssAcfFitTapsIn),
                                    C.POINTER(GnssAcfFitOut)]),
    "gnss_acf_fit_taps_window": (C.c_int, [C.POINTER(GnssAcfFitTapsCfg), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(GnssAcfFitOut)]),
    # the delay-Doppler map over replayed rows (additive within ABI v14: detected by symbol)
    "gnss_replay_ddm": (C.c_int, [C.c_void_p, C.POINTER(GnssReplayDdmCfg), C.POINTER(GnssReplayDdmIn),
                                  C.POINTER(GnssReplayDdmOut)]),
    # the multi-ray fit on any tap grid (additive within ABI v14: detected by symbol)
    "gnss_acf_fit_multi": (C.c_int, [C.c_void_p, C.POINTER(GnssAcfFitMultiCfg), C.POINTER(GnssAcfFitTapsIn),
                                     C.POINTER(GnssAcfFitMultiOut)]),
    "gnss_acf_fit_multi_window": (C.c_int, [C.POINTER(GnssAcfFitMultiCfg), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(GnssAcfFitMultiOut)]),
    "gnss_lane_boundaries": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double]),
    "gnss_ctx_lane_path": (C.c_int, [C.c_void_p]),
}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libgnss_mi355x.so")
_lib = None
_torch_first = False
LOADED_PATH = None  # the library file the process bound (bench.py digests it)

# gnss_ctx_set_option keys (include/gnss_mi355x.h, ABI v11)
(OPT_FORCE_SUB, OPT_NO_PERSIST, OPT_FORCE_VPB, OPT_ACQ_ROCFFT, OPT_FINE_ROCFFT, OPT_ACQ_BATCH, OPT_ACQ_FUSED,
 OPT_ACQ_RING, OPT_ACQ_PIPE, OPT_VT_BLOCKS, OPT_FORCE_PEER, OPT_VT_SPAN, OPT_SLOT_PATH) = range(13)
MAX_DEVICES = 16


def require_torch():
    """torch, for the entry points that exchange device tensors with the library; raises if
    the library was loaded before torch (torch would then see no GPU in this process)."""
    import torch
    if _lib is not None and not _torch_first:
        raise RuntimeError("import torch before the first gnss Context / abi.load() "
                           "(PyTorch-ROCm must bring up its HIP runtime first)")
    return torch


class GnssError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__(f"gnss status {status}: {msg}")


def load(path: str | None = None):
    """Load the HIP C-ABI library (raises if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # GNSS_LIB: a timing-probe build (tools/build_probe.sh) in place of the product library
    p = path or os.environ.get("GNSS_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} missing: the HIP extension is not built "
                          "(run `python -c 'import __graft_entry__ as g; g.build()'`)")
    # PyTorch-ROCm ships its own HIP / HSA runtime and finds no GPU if this library's runtime
    # came up first, so it is imported here, before the library, whenever it is installed: a
    # caller may create a Context first and hand tensors over later (device-resident outputs,
    # the RCCL gathers). require_torch() still checks the order for a library loaded without
    # torch installed at the time.
    global _torch_first
    if _lib is None:
        if "torch" not in sys.modules and os.environ.get("GNSS_NO_TORCH", "0") != "1":
            try:  # PyTorch's runtime first: any later tensor exchange then works
                import torch  # noqa: F401
            except Exception:  # (a torch that fails to import, e.g. an OSError from its ROCm
                pass  # libraries, must not stop the GNSS library from loading; require_torch() checks)
        _torch_first = "torch" in sys.modules
    lib = C.CDLL(p)
    for name, (res, args) in PROTOTYPES.items():
        if p != LIB_PATH and not hasattr(lib, name):
            continue  # (an A/B or probe build of another revision: entry points it lacks stay unbound)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        global LOADED_PATH
        _lib = lib
        LOADED_PATH = os.path.abspath(p)
    return lib
