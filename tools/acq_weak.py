#!/usr/bin/env python3
"""Weak-signal acquisition on a recording: the reference's coherent 4-ms search beside the
non-coherent one (gpsmi_acq_search_nc), per SV.

    python tools/acq_weak.py <recording.bin> [--start-stream K] [--n-coh 4] [--n-seg 25] [--json]

    <recording.bin>   u8 IQ as gpsbin.py records it and streamData reads it (gpsrecv.py:162-173),
                      2.048 Msps.  Read with ingest.read_raw_blocks (START_STREAM honoured) and
                      decoded on the GPU (raw input format).

The coherent search is sweepAllSats's surface (gpsrecv.py:241-274): 31 SV x 50 bins
(-5000 .. +4800 step 200) x SWEEP_CORR_AVG = 4 ms on the first block.  The weak search is
Acquisition.sweepWeakSats over the same SVs and bins on the first n_seg * n_coh ms: the mean of
the correlation magnitudes of n_seg segments of n_coh ms.  Per SV both print the best
normMaxCorr over the bins, its bin and code phase, and whether it passes CORR_MIN (the weak
search claims an SV at the first bin over CORR_MIN, as sweepAllSats does); the device time of
each search (gpsmi_acq_last_ms) closes the report.  --json prints one JSON object instead."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gps-sdr-receiver_amd'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('recording')
    ap.add_argument('--start-stream', type=int, default=0)
    ap.add_argument('--n-coh', type=int, default=4)
    ap.add_argument('--n-seg', type=int, default=25)
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args(argv)

    from gpsmi import ingest
    from gpsmi.acquisition import Acquisition, SAT_ALL, norm_max_corr
    acq = Acquisition(raw_u8=True)
    cfg = acq.cfg
    need = a.n_seg * a.n_coh * cfg.code_samples
    blocks = []
    for raw in ingest.read_raw_blocks(a.recording, cfg.ngps, a.start_stream):
        blocks.append(raw)
        if len(blocks) * cfg.ngps >= need:
            break
    if len(blocks) * cfg.ngps < need:
        sys.exit(f'{a.recording}: {len(blocks) * cfg.ngps} samples after stream '
                 f'{a.start_stream}, the weak search needs {need}')
    data = np.concatenate(blocks)[:need]
    freqs = [cfg.min_freq + cfg.step_freq * i
             for i in range(int(round((cfg.max_freq - cfg.min_freq) / cfg.step_freq)))]
    prns = list(SAT_ALL)

    def best(table):
        rows = []
        for j, s in enumerate(prns):
            nmc = [norm_max_corr(table[b, j]) for b in range(len(freqs))]
            b = int(np.argmax(nmc))
            rows.append(dict(prn=s, nmc=float(nmc[b]), freq=freqs[b],
                             code_phase=int(table[b, j]['argmax'])))
        return rows

    avg = min(cfg.sweep_corr_avg, cfg.n_cyc)
    coh = best(acq.engine.search(blocks[0], prns, freqs, avg))
    coh_ms = acq.engine.last_ms()
    for r in coh:
        r['found'] = r['nmc'] > cfg.corr_min
    weak = best(acq.engine.search_noncoherent(data, prns, freqs, a.n_coh, a.n_seg))
    found = acq.sweepWeakSats(data, freqs, list(prns), [], n_coh=a.n_coh, n_seg=a.n_seg)
    weak_ms = acq.engine.last_ms()
    claim = {s: (f, d, nmc) for nmc, s, f, d in found}
    for r in weak:
        r['found'] = r['prn'] in claim
        if r['found']:           # the first-hit bin and code phase, as sweepAllSats reports them
            r['freq'], r['code_phase'], r['nmc'] = claim[r['prn']][0], claim[r['prn']][1], \
                float(claim[r['prn']][2])
    acq.engine.close()
    rep = dict(recording=a.recording, start_stream=a.start_stream, n_coh=a.n_coh,
               n_seg=a.n_seg, coherent_ms=coh_ms, weak_ms=weak_ms, coherent=coh, weak=weak)
    if a.json:
        print(json.dumps(rep))
        return
    print(f'{"PRN":>4} | {"4 ms: nmc":>10} {"bin Hz":>7} {"phase":>5} | '
          f'{a.n_seg} x {a.n_coh} ms: {"nmc":>6} {"bin Hz":>7} {"phase":>5}')
    for c, w in zip(coh, weak):
        mark = lambda r: '*' if r['found'] else ' '
        print(f'{c["prn"]:>4} | {c["nmc"]:>9.2f}{mark(c)} {c["freq"]:>7.0f} {c["code_phase"]:>5} | '
              f'{"":>13}{w["nmc"]:>6.2f}{mark(w)} {w["freq"]:>7.0f} {w["code_phase"]:>5}')
    print(f'* = over CORR_MIN {cfg.corr_min:g}.  device time: 4-ms search {coh_ms:.3f} ms, '
          f'{a.n_seg} x {a.n_coh} ms search {weak_ms:.3f} ms')


if __name__ == '__main__':
    main()
