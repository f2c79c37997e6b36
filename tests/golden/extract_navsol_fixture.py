"""Extract tests/golden/ref_navSolCT_10ms_Opensky.npz: the positioning half of
trackingCT_POS_updated.m (:147-171, :420-565) as the reference recorded it on the real Opensky IF.

    python tests/golden/extract_navsol_fixture.py <path to the reference's SDR_MATLAB-main>

Reads the reference's result files (read-only) and writes data only:

  INPUT   tckRstCT_10ms_Opensky.mat   TckResultCT_pos(prn).absoluteSample / remChip / codeFreq /
                                      carrFreq, 5 PRNs x 3000 steps (the four series :427-457,514 read)
          nAcquired_Opensky_5000.mat  sv (channel order)
          countinx.mat                countinx, read by channel POSITION (:29,183, quirk A.17)
          eph_Opensky_40.mat          the 21 svPosVel.m values at eph_idx 1, sfb(1), TOW(1)
          sbf_Opensky_40.mat          nav1(prn)
  OUTPUT  navSolCT_10ms_Opensky.mat   every navSolutionsCT field of :509-551, 660 rows

sampleStartMea (:160) needs TckResult_Eph, which the reference does not ship. It is derived here:
the one sample position at which row 1's five codePhaseMeas (:452-453) come out bit for bit. The
script finds every such position and asserts that there is exactly one.

Only scipy.io.loadmat (a MAT-v5 parser that executes nothing) is used.
"""
import os
import sys

import numpy as np
import scipy.io as sio

HERE = os.path.dirname(os.path.abspath(__file__))
EPH_SV_FIELDS = ["sqrta", "deltan", "toe", "M0", "ecc", "w", "Cus", "Cuc", "Crs", "Crc", "Cis", "Cic", "i0",
                 "idot", "omegae", "omegadot", "toc", "af0", "af1", "af2", "TGD"]
SOL_FIELDS = ["rawPseudorange", "usrPos", "usrVel", "usrPosENU", "usrPosLLH", "clkBias", "usrVelENU", "clkDrift",
              "DOP", "satEA", "satAZ", "timeTransmit", "codePhaseMeas", "localTime"]
FS, DATATYPE = 58e6, 2


def code_phase_meas(absS, remChip, codeFreq, curr):
    """:442-453 for one channel at measurement sample `curr` -> (index, codePhaseMeas) or None."""
    first = int(np.searchsorted(absS, curr, side="right")) + 1  # 1-based first i with absS(i) > curr
    if first > absS.size or first < 2:
        return None
    i = first - 2  # 0-based `index`
    return first - 1, remChip[i] + (codeFreq[i] / FS) * ((curr - absS[i]) / DATATYPE)


def find_sample_start(rec, cpm_row1):
    """Every integer sample position whose five codePhaseMeas equal row 1's bit for bit."""
    a0, r0, f0 = rec["absoluteSample"][0], rec["remChip"][0], rec["codeFreq"][0]
    hits = set()
    for i in range(a0.size - 1):  # channel 1 inverts (:452-453) per candidate `index`
        guess = a0[i] + DATATYPE * (cpm_row1[0] - r0[i]) / (f0[i] / FS)
        for curr in np.round(guess) + np.arange(-3, 4):
            if not a0[i] <= curr < a0[i + 1]:
                continue
            ok = True
            for s in range(len(cpm_row1)):
                m = code_phase_meas(rec["absoluteSample"][s], rec["remChip"][s], rec["codeFreq"][s], curr)
                ok = ok and m is not None and m[1] == cpm_row1[s]
            if ok:
                hits.add(int(curr))
    return sorted(hits)


def main(ref):
    ld = lambda f, k: sio.loadmat(os.path.join(ref, f), squeeze_me=True, struct_as_record=False)[k]
    sv = [int(p) for p in np.atleast_1d(ld("nAcquired_Opensky_5000.mat", "nAcquired").sv)]
    ct = ld("tckRstCT_10ms_Opensky.mat", "TckResultCT_pos")
    ns = ld("navSolCT_10ms_Opensky.mat", "navSolutionsCT")
    eph = ld("eph_Opensky_40.mat", "eph")
    sbf = ld("sbf_Opensky_40.mat", "sbf")
    cx = np.atleast_1d(ld("countinx.mat", "countinx")).astype(np.int64)
    out = {"prns": np.array(sv), "countinx": cx[: len(sv)]}
    rec = {}
    for f in ("absoluteSample", "remChip", "codeFreq", "carrFreq"):
        rec[f] = np.stack([np.asarray(getattr(ct[p - 1], f), dtype=np.float64).ravel() for p in sv])
        out["rec_" + f] = rec[f]
    out["nav1"] = np.array([int(np.atleast_1d(sbf.nav1)[p - 1]) for p in sv], dtype=np.int64)
    out["sfb1"] = np.array([int(np.atleast_1d(eph[p - 1].sfb)[0]) for p in sv], dtype=np.int64)   # eph(prn).sfb(1)
    out["TOW1"] = np.array([float(np.atleast_1d(eph[p - 1].TOW)[0]) for p in sv])                  # eph(prn).TOW(1)
    out["eph"] = np.array([[float(np.atleast_1d(getattr(eph[p - 1], f))[0]) for f in EPH_SV_FIELDS] for p in sv])
    n = len(sv)
    for f in SOL_FIELDS:
        v = np.asarray(getattr(ns, f), dtype=np.float64)
        out["sol_" + f] = v.reshape(v.shape[0], -1) if v.ndim > 1 else v.ravel()
    rows = out["sol_localTime"].size
    assert out["sol_codePhaseMeas"].shape == (rows, n) and out["sol_usrPos"].shape == (rows, 3)
    hits = find_sample_start(rec, out["sol_codePhaseMeas"][0])
    assert len(hits) == 1, hits
    out["sampleStartMea"] = np.array(hits[0], dtype=np.int64)
    path = os.path.join(HERE, "ref_navSolCT_10ms_Opensky.npz")
    np.savez_compressed(path, **out)
    print("prns", sv, "rows", rows, "sampleStartMea", hits[0], "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
