"""MANUAL (MI355X): what vg_pg_optimize costs.  256 pose graphs of 1000 keyframes with 100 loop edges in ONE call, and one such graph
alone.  One allocating call, reported on its own, then three repeats: wall time of the C call (the Python packing outside the timed region)
and the device time of the launch from events (vg_pg_out::device_ms).  The stage is latency-bound by design: a graph keeps one CU busy, its
two triangular sweeps per conjugate-gradient iteration are a chain of 4 n_free dependent steps, and throughput comes from the batch; the
number that bounds it is the time per block row (4 scalar rows) of a sweep, reported as an upper bound: the whole device time of the single
graph over (sweeps x n_free).  There is no earlier device version; next to it stands the time of the float64 RESTATEMENT's dense64 route
(tests/kf_pgo_ref.py: numpy, dense LM system, numpy.linalg.solve) for the same graph on the same box -- a restatement, not Ceres.

usage: python tests/manual/gpu_kf_pgo.py [--out profiles/kf_pgo.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_GRAPHS, N_KF, N_LOOPS, REPEATS = 256, 1000, 100, 3


def graph(K, seed):
    loops = [(500 + 5 * k - (k % 3), 5 * k + 2) for k in range(N_LOOPS)]
    loops[-1] = (N_KF - 1, loops[-1][1])
    return K.scene(seed, N_KF, loops, noise=0.05)


def timed(fe, h, graphs):
    L = fe.pg_lib(h)
    n = len(graphs)
    ins, outs = (fe.PgIn * n)(), (fe.PgOut * n)()
    keep = [fe.pg_fill(L, ins[i], outs[i], g) for i, g in enumerate(graphs)]
    ms = np.zeros(fe.PG_LAUNCHES, np.float32)
    outs[0].device_ms = ms.ctypes.data_as(fe._f4)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = L.vg_pg_optimize(h.h, n, ins, outs)
        assert rc == 0, rc
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append([float(x) for x in ms])
    its = [int(o.iterations) for o in outs]
    cg = [[int(o.it_cg[k]) for k in range(o.iterations)] for o in outs]
    d = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], device_ms_per_launch=dev[1:], statuses_ok=[int(o.status) for o in outs].count(0),
             iterations_min_max=[min(its), max(its)], cg_iterations_min_max=[min(min(c) for c in cg), max(max(c) for c in cg)],
             n_free=int(outs[0].n_free), n_edges=int(outs[0].n_edges), n_loop_edges=int(outs[0].n_loop_edges))
    return d, outs, cg, keep


def run():
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba, fe
    import kf_pgo_ref as K
    h = ba.Handle()
    res = dict(what=f"vg_pg_optimize, {N_GRAPHS} graphs of {N_KF} keyframes with {N_LOOPS} loop edges; one allocating call, then {REPEATS} repeats",
               launches=fe.PG_KERNELS, note="latency-bound by design: one graph keeps one CU busy, throughput comes from the batch")
    graphs = [graph(K, 3000 + i) for i in range(N_GRAPHS)]
    res["batch"], _, _, _ = timed(fe, h, graphs)
    res["one_graph"], outs, cg, _ = timed(fe, h, graphs[:1])
    sweeps = sum(2 * (c + 1) for c in cg[0])
    one_ms = min(x[0] for x in res["one_graph"]["device_ms_per_launch"])
    res["one_graph"]["sweeps"] = sweeps
    res["one_graph"]["factorisations"] = len(cg[0])
    res["one_graph"]["us_per_block_row_of_a_sweep_upper_bound"] = one_ms * 1e3 / (sweeps * res["one_graph"]["n_free"])
    res["batch"]["device_ms_per_graph"] = [x[0] / N_GRAPHS for x in res["batch"]["device_ms_per_launch"]]
    t0 = time.perf_counter()
    ref = K.solve(graphs[0], 'dense64')
    res["cpu_restatement_dense64_s"] = time.perf_counter() - t0
    assert (outs[0].status, outs[0].termination, outs[0].iterations) == (ref['status'], ref['termination'], ref['iterations'])
    res["one_graph"]["final_cost_device_vs_restatement"] = [float(outs[0].final_cost), float(ref['final_cost'])]
    h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run()
    print(json.dumps(r, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
