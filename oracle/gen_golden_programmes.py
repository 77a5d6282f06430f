#!/usr/bin/env python3
"""Generate tests/golden/programmes.json by running the REAL reference (oracle/_ref/libiamf_ref.so) over the structured
programmes of tests/programmes.py.

TEST INFRASTRUCTURE, the recipe of gen_golden.py (whose ctypes set-up it reuses): runs only where the reference has been
compiled (`make -C oracle ref`).  Stored per case: the parameters, the output's length and the sha256 of its bytes, not
the waveform.  NaN payloads and signs are canonicalised before hashing (programmes.canonical_bytes): every NaN counts
as 0x7fc00000, its position still counts.  manifest.json is not touched.
  audio_effect_peak_limiter_*    src/iamf_dec/audio_effect_peak_limiter.c   (limiter programmes, 2 channels)
  demixer_*                      src/iamf_dec/demixer.c                     (demixer programmes, stereo -> 5.1.2 -> 7.1.4)
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import demix_cases as D  # noqa: E402
import gen_golden as GG  # noqa: E402  (loads the reference; its main() is not run)
import programmes as P  # noqa: E402

NOTE = ("sha256 over the float32 output bytes ([ch][n] for the limiter, [frames][ch][fs] for the demixer) of the real "
        "reference; every NaN is replaced by the quiet NaN 0x7fc00000 before hashing (payloads and signs of NaN are not "
        "pinned, their positions are)")


def call_sizes(n, call):
    return [call] * (n // call) + ([n % call] if n % call else [])


PLATEAU_DB = (0, -6)     # the plateau pair's other thresholds: 0 dB is 1.0f exactly


def limiter_cases():
    """(key, programme name, extra arguments, rate, n, samples per call[, threshold in dB])"""
    out = []
    for f in P.LIMITER:
        if f is P.release_to_idle:
            continue
        for call in (1024, 960):
            out.append(("limiter/%s/c%d" % (f.__name__, call), f.__name__, {}, 48000, 6144, call))
    for rate in P.RATES:
        for call in (1024, 960) if rate == 48000 else (1024,):
            out.append(("limiter/release_to_idle/%d/c%d" % (rate, call), "release_to_idle", {}, rate,
                        1024 * P.RELEASE_FRAMES[rate], call))
    for k in range(P.SWEEP):
        for call in (1024, 960):
            out.append(("limiter/retrigger_sweep/k%d/c%d" % (k, call), "retrigger_sweep", {"k": k}, 48000, 12288, call))
    # the other rates of tests/test_gpu_rates.py: the full release and the eight re-trigger positions at frames(rate) frames
    for rate in P.SWEEP_RATES:
        n = 1024 * P.frames(rate)
        out.append(("limiter/release_to_idle/%d/f%d/c1024" % (rate, P.frames(rate)), "release_to_idle", {}, rate, n, 1024))
        for k in range(P.SWEEP):
            out.append(("limiter/retrigger_sweep/%d/k%d/c1024" % (rate, k), "retrigger_sweep", {"k": k}, rate, n, 1024))
    for rate in (48000,) + P.SWEEP_RATES:      # chunks that start inside the attack
        out.append(("limiter/attack_across_chunks/%d/c1024" % rate, "attack_across_chunks", {}, rate, 1024 * max(P.frames(rate), 4), 1024))
    for db in PLATEAU_DB:
        for name in ("dc_at_threshold", "dc_one_ulp_above"):
            out.append(("limiter/%s/%ddB/c1024" % (name, db), name, {"db": float(db)}, 48000, 6144, 1024, float(db)))
    return out


def digest(a):
    return hashlib.sha256(P.canonical_bytes(a)).hexdigest()


def main():
    pins = {"_note": NOTE}
    with np.errstate(all="ignore"):
        for key, name, args, rate, n, call, *thr_db in limiter_cases():
            x = getattr(P, name)(2, n, rate, **args)
            y, _ = GG.ref_limiter(x, call_sizes(n, call), rate=rate, **({"thr_db": thr_db[0]} if thr_db else {}))
            pins[key] = dict(programme=name, args=args, ch=2, rate=rate, n=n, call=call, out_len=int(y.shape[1]),
                             sha256=digest(y), **({"thr_db": thr_db[0]} if thr_db else {}))
        c = P.demix_case(1024)
        for f in P.DEMIXER:
            y = D.drive_demixer(GG.ref, "demixer_", c, P.demix_input(f, c))
            pins["demix/" + f.__name__] = dict(programme=f.__name__, fs=1024, frames=int(y.shape[0]), ch=int(y.shape[1]),
                                               out_len=int(y.size), sha256=digest(y))
    with open(os.path.join(ROOT, "tests", "golden", "programmes.json"), "w") as fh:
        json.dump(pins, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d reference results pinned in tests/golden/programmes.json" % (len(pins) - 1))


if __name__ == "__main__":
    main()
