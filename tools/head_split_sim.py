#!/usr/bin/env python3
"""Event model of the synchronous host call with a head (option "head_queries"): where does a 10 k batch end for a given H?  (CPU only)

    python tools/head_split_sim.py [nq [H ...]]

The chip holds SLOTS one-wave walks; a hop takes HOP_IDLE us on an empty chip and HOP_FULL us on a full one, linear in between
(profiles/r06_hop_phases.txt).  Walk lengths: mean 133 hops, p99 about 165, p99.9 about 195 and one outlier of 219..263 per batch
(profiles/r05_host_phases.txt, r05_outlier_walks.txt).  The main part starts when its pre-pass ends (the whole batch's bytes over
the link, PREPASS_US for 10 k queries) and is launched in the order of a key whose correlation with the hop count is 0.57; a head
query starts when its row has crossed the link (row i at LINK_LAT_US + i * 512 B / 54 GB/s).  Not modelled: the second launch and
the join, head walks competing with descent waves for slots and for the memory system -- the measured gain is smaller
(profiles/head_split_ab.txt)."""
import sys

import numpy as np

SLOTS, HOP_IDLE, HOP_FULL = 8192, 0.79, 1.3
LINK_LAT_US, ROW_US, PREPASS_US, CORR, DT = 28.0, 512 / 54e3, 122.0, 0.57, 0.25


def batch(rng, nq):
    hops = rng.normal(133.0, 12.5, nq)
    wide = rng.random(nq) < 0.015
    hops[wide] = rng.normal(150.0, 20.0, int(wide.sum()))
    hops = np.maximum(hops, 60.0)
    hops[rng.integers(0, nq)] = rng.uniform(219.0, 263.0)
    return hops


def step_end(rng, nq, H):
    hops = batch(rng, nq)
    start = np.empty(nq)
    start[:H] = LINK_LAT_US + ROW_US * np.arange(1, H + 1)
    z = (hops[H:] - hops[H:].mean()) / hops[H:].std()
    key = CORR * z + np.sqrt(1 - CORR * CORR) * rng.standard_normal(nq - H)
    order = np.concatenate([np.arange(H), H + np.argsort(-key)])           # the launch order: head rows, then the main part by key
    start[H:] = LINK_LAT_US + (PREPASS_US - LINK_LAT_US) * nq / 10_000         # (all nq rows cross the one link, whoever reads them)
    left = hops.copy()
    running = np.zeros(nq, bool)
    nxt, t, done = 0, 0.0, 0
    while done < nq:
        free = SLOTS - int(running.sum())
        while nxt < nq and free > 0 and start[order[nxt]] <= t:             # (in launch order: a block waits for the one in front)
            running[order[nxt]] = True
            nxt += 1
            free -= 1
        r = int(running.sum())
        if r:
            left[running] -= DT / (HOP_IDLE + (HOP_FULL - HOP_IDLE) * r / SLOTS)
            fin = running & (left <= 0)
            done += int(fin.sum())
            running &= ~fin
        t += DT
    return t


if __name__ == "__main__":
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
    heads = [int(a) for a in sys.argv[2:]] or [0, max(nq - SLOTS, 0), int(0.3 * nq), int(0.4 * nq), int(0.5 * nq)]
    for H in heads:
        ends = [step_end(np.random.default_rng(7 + b), nq, H) for b in range(6)]
        print("nq %d  H %5d: step end %.0f us (mean of 6 batches, before the fixed cost of the call)" % (nq, H, float(np.mean(ends))))
