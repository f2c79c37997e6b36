"""Vectorised numpy restatement of one step of trackingVT_POS_updated_multicorrelator.m's
tracking half (:151-470; test infrastructure): the expected side of the 25-tap vector-tracking
tests, built on numpy_twin's colon / ca_code / read_samples. It follows the reference line by
line -- Spacing = 0.6:-0.05:-0.6 (:26), Code = [c(end) c(end-1) repmat(c,1,pdi) c(1) c(2)]
(:104) indexed Code(ceil(t) + 2) (:256-281), the per-sample Wave (:285-291), the 50 sums
(:301-350, each summed in long double) and the scalar end (:354-391) -- and raises IndexError
where MATLAB raises (a table index out of range, operands of .* of different lengths)."""
import math

import numpy as np

from numpy_twin import ca_code, colon, read_samples

NTAPS = 25
E, P, L = 2, 12, 22  # Spacing(3) / (13) / (23), 0-based


def spacing():
    return colon(0.6, -0.05, -0.6)


def code_table(prn, pdi=1):
    c = ca_code(prn)
    return np.concatenate([[c[-1], c[-2]], np.tile(c, pdi), [c[0], c[1]]])


def loop_coef(LBW, zeta, k):
    """calcLoopCoef.m:41-45."""
    Wn = LBW * 8 * zeta / (4 * (zeta * zeta) + 1)
    return k / (Wn * Wn), 2.0 * zeta / Wn


def new_state(file_ptr, remChip, remCarrPhase, codeFreq, carrFreq, carrFreqBasis, oldCarrNco=0.0,
              oldCarrError=0.0):
    return dict(file_ptr=int(file_ptr), remChip=float(remChip), remCarrPhase=float(remCarrPhase),
                codeFreq=float(codeFreq), carrFreq=float(carrFreq), carrFreqBasis=float(carrFreqBasis),
                oldCarrNco=float(oldCarrNco), oldCarrError=float(oldCarrError), index_int=0, snrIndex=1,
                Zk=np.zeros(20))


def num_sample(st, Fs=58e6, codelength=1023.0, pdi=1):
    return math.ceil((codelength * pdi - st["remChip"]) / (st["codeFreq"] / Fs))  # :155


def tap_colons(st, cf_new, n, Fs=58e6):
    """The 25 colons of :230-254 (each must have n elements for the .* of :301-350)."""
    cps = cf_new / Fs
    out = []
    for s in spacing():
        t = colon((0 + s) + st["remChip"], cps, ((n - 1) * cps + s) + st["remChip"])
        if len(t) != n:
            raise IndexError("colon length")
        out.append(t)
    return out


def correlate(buf, st, cf_new, prn, Fs=58e6, codelength=1023.0, pdi=1, prec=1, dtype=2, table=None):
    """:155-350 -> (n, tap_i[25], tap_q[25], t_prompt, Wave). buf = the record's bytes (int8 view,
    byte 0 = file byte 0)."""
    n = num_sample(st, Fs, codelength, pdi)
    if n < 1:
        raise IndexError("numSample")
    bps = prec * dtype
    if st["file_ptr"] + n * bps > buf.size:
        raise EOFError("short fread")
    raw = read_samples(buf[st["file_ptr"]:], prec, dtype, n)
    Code = code_table(prn, pdi) if table is None else table
    ts = tap_colons(st, cf_new, n, Fs)
    Wave = (2 * np.pi * (st["carrFreq"] * (np.arange(0, n + 1) / Fs))) + st["remCarrPhase"]  # :285-286
    prod = raw * np.exp(1j * Wave[:n])
    I = np.imag(prod).astype(np.longdouble)
    Q = np.real(prod).astype(np.longdouble)
    ti, tq = np.zeros(NTAPS), np.zeros(NTAPS)
    for j, t in enumerate(ts):
        idx = np.ceil(t).astype(np.int64) + 2  # 1-based (:256)
        if idx.min() < 1 or idx.max() > Code.size:
            raise IndexError("Code index")
        code = Code[idx - 1]
        ti[j] = float(np.sum(code * I))
        tq[j] = float(np.sum(code * Q))
    return n, ti, tq, ts[P], Wave


def finish(st, cf_new, n, ti, tq, t_prompt, Wave, Fs=58e6, ms=1e-3, pdi=1, pll=(15, 0.707, 0.25), bps=2):
    """:354-391, :462-470 from the sums -> the step's record; advances st."""
    t1, t2 = loop_coef(*pll)
    cps = cf_new / Fs
    remChip = (t_prompt[n - 1] + cps) - 1023 * pdi
    remCarrPhase = math.fmod(Wave[n], 2 * np.pi)
    r = dict(tap_i=ti.copy(), tap_q=tq.copy(), E_i=ti[E], E_q=tq[E], P_i=ti[P], P_q=tq[P], L_i=ti[L], L_q=tq[L],
             CN0=0.0, cn0_row=0)
    st["index_int"] += 1
    st["Zk"][st["index_int"] - 1] = r["P_i"] ** 2 + r["P_q"] ** 2
    if st["index_int"] % 20 == 0:
        m = np.mean(st["Zk"])
        v = np.var(st["Zk"], ddof=1)
        NA2 = np.sqrt(complex(m * m - v))
        varIQ = 0.5 * (m - NA2)
        r["CN0"] = float(abs(10 * np.log10(1 / (1 * ms * pdi) * NA2 / (2 * varIQ))))
        r["cn0_row"] = st["snrIndex"]
        st["index_int"] = 0
        st["snrIndex"] += 1
    carrError = math.atan(r["P_q"] / r["P_i"]) / (2.0 * np.pi)
    carrNco = st["oldCarrNco"] + (t2 / t1) * (carrError - st["oldCarrError"]) + carrError * (pdi * 1e-3 / t1)
    carrFreq = st["carrFreqBasis"] + carrNco
    Ee = math.sqrt(r["E_i"] ** 2 + r["E_q"] ** 2)
    Ll = math.sqrt(r["L_i"] ** 2 + r["L_q"] ** 2)
    absS = st["file_ptr"] + n * bps
    r.update(codeError=-0.5 * (Ee - Ll) / (Ee + Ll), carrError=carrError, carrNco=carrNco, remChip=remChip,
             remCarrPhase=remCarrPhase, codeFreq=cf_new, carrFreq=carrFreq, numSample=n, absoluteSample=absS,
             codedelay=math.fmod(absS / bps, Fs * ms))
    st.update(file_ptr=absS, remChip=remChip, remCarrPhase=remCarrPhase, codeFreq=cf_new, carrFreq=carrFreq,
              oldCarrNco=carrNco, oldCarrError=carrError)
    return r


def step(buf, st, cf_new, prn, Fs=58e6, codelength=1023.0, ms=1e-3, pdi=1, pll=(15, 0.707, 0.25), prec=1, dtype=2,
         table=None):
    """One whole step of channel `prn` -> its record (a dict); st advanced in place."""
    n, ti, tq, tp, Wave = correlate(buf, st, cf_new, prn, Fs, codelength, pdi, prec, dtype, table)
    return finish(st, cf_new, n, ti, tq, tp, Wave, Fs, ms, pdi, pll, prec * dtype)
