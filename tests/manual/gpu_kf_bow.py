"""MANUAL (MI355X): what vg_kf_loop_detect costs.  A synthetic k = 10, L = 6 vocabulary generated here (1,111,110 nodes x 32 B = 35.6 MB of
descriptors: random descriptors, positive random weights), 256 databases each pre-filled with 500 entries of 5000 random descriptors, then
ONE call of 256 requests (query + add; frame_index makes every entry eligible) and a one-request call.  One allocating call, reported on
its own, then three repeats: wall time of the C call (the Python packing outside the timed region) and the device time of each launch from
events (vg_bow_out::device_ms).  The walk kernel's achieved rate counts descriptors x sibling groups fetched (L groups of k x 32 B each)
against the Infinity-Cache gather rate of a 38 MB table.  The project has no host detectLoop to compare with: no speed-up is claimed.

Random descriptors against a random tree share few words (about n^2 / 10^6 per pair of frames), so the score kernel's intersections find
little: its time here is the bisection over the entries' words, not the chain.

usage: python tests/manual/gpu_kf_bow.py [--out profiles/kf_bow.json] [--rehearse]   (--rehearse: a toy size on whatever library is loaded)"""
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
REPEATS = 3


def uniform_voc(fe, k, L, seed=1):
    """breadth-first ids: the children of node p are p k + 1 .. p k + k; the leaves are the last k^L ids"""
    rng = np.random.default_rng(seed)
    n = (k ** (L + 1) - 1) // (k - 1) - 1
    first_leaf = (k ** L - 1) // (k - 1)
    nodes = np.zeros(n, fe.VOC_NODE)
    ids = np.arange(1, n + 1, dtype=np.int64)
    nodes["node_id"], nodes["parent_id"] = ids, (ids - 1) // k
    nodes["descriptor"] = rng.integers(0, 2 ** 63, (n, 4), dtype=np.int64).astype(np.uint64) << np.uint64(1) | rng.integers(0, 2, (n, 4), dtype=np.int64).astype(np.uint64)
    nodes["weight"][first_leaf - 1:] = rng.uniform(0.5, 9.0, n - first_leaf + 1)
    words = np.zeros(n - first_leaf + 1, fe.VOC_WORD)
    words["node_id"], words["word_id"] = ids[first_leaf - 1:], np.arange(len(words))
    return nodes, words


def run(rehearse, handle=None):
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba, fe
    import kf_brief_ref as KB
    k, L, n_db, n_fill, n_desc, n_slots = (10, 3, 4, 5, 200, 8) if rehearse else (10, 6, 256, 500, 5000, 512)
    h = handle or ba.Handle()
    lib = fe._bow_lib(h)
    rng = np.random.default_rng(7)
    nodes, words = uniform_voc(fe, k, L)
    t0 = time.perf_counter()
    fe.voc_load(h, k, L, nodes, words)
    t_load = time.perf_counter() - t0
    kf = fe.KeyFrames(h, 67, 41, n_desc, 8, n_slots, KB.pattern())
    fe.bow_configure(h, n_db, n_fill + 8, (n_fill + 8) * n_desc)
    zero2, zero1 = np.zeros((n_desc, 2), np.float32), np.zeros(n_desc, np.uint8)
    for s in range(n_slots):
        d = rng.integers(0, 2 ** 63, (n_desc, 4), dtype=np.int64).astype(np.uint64) << np.uint64(1) | rng.integers(0, 2, (n_desc, 4), dtype=np.int64).astype(np.uint64)
        kf.set(s, zero2, zero1, zero2, d, np.zeros((0, 2), np.float32), np.zeros((0, 4), np.uint64))

    def structs(reqs):
        n = len(reqs)
        ins, outs = (fe.BowIn * n)(), (fe.BowOut * n)()
        for i, (db, slot, fi, fl) in enumerate(reqs):
            ins[i].struct_size, ins[i].db, ins[i].slot, ins[i].frame_index, ins[i].flags = C.sizeof(fe.BowIn), db, slot, fi, fl
            outs[i].struct_size = C.sizeof(fe.BowOut)
        return ins, outs

    t0 = time.perf_counter()
    for j in range(n_fill):                                                      # 13 and n_slots are coprime: a database never sees a slot twice
        ins, outs = structs([(db, (db * 7 + j * 13) % n_slots, j, fe.BOW_ADD) for db in range(n_db)])
        assert lib.vg_kf_loop_detect(h.h, n_db, ins, outs) == 0, h.lib.vg_last_error(h.h)
    t_fill = time.perf_counter() - t0
    words_per_entry = fe.bow_count(h, 0)[1] / n_fill

    def timed(reqs_of_rep):
        ms = np.zeros(fe.BOW_LAUNCHES, np.float32)
        wall, dev, last = [], [], None
        for rep in range(REPEATS + 1):
            ins, outs = structs(reqs_of_rep(rep))
            outs[0].device_ms = ms.ctypes.data_as(fe._f4)
            t = time.perf_counter()
            rc = lib.vg_kf_loop_detect(h.h, len(ins), ins, outs)
            wall.append((time.perf_counter() - t) * 1e3)
            assert rc == 0, h.lib.vg_last_error(h.h)
            dev.append([float(x) for x in ms])
            last = outs
        return dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], call_wall_ms_min_max=[min(wall[1:]), max(wall[1:])], device_ms_per_launch=dev[1:],
                    device_ms_total=[sum(x) for x in dev[1:]], n_results_min_max=[min(int(o.n_results) for o in last), max(int(o.n_results) for o in last)],
                    n_words_min_max=[min(int(o.n_words) for o in last), max(int(o.n_words) for o in last)])

    fi = n_fill + 60                                                             # max_id = frame_index - 50 admits every entry
    res = dict(what=f"vg_kf_loop_detect, k = {k}, L = {L} vocabulary ({len(nodes)} nodes, {32 * len(nodes) / 1e6:.1f} MB of descriptors), {n_db} databases of "
                    f"{n_fill} entries of {n_desc} descriptors ({words_per_entry:.0f} words an entry); one allocating call, then {REPEATS} repeats",
               launches=fe.BOW_KERNELS, voc_load_s=t_load, fill_s=t_fill)
    res["batch_query_add"] = timed(lambda rep: [(db, (db * 5 + rep) % n_slots, fi + rep, fe.BOW_QUERY | fe.BOW_ADD) for db in range(n_db)])
    res["one_request_query_add"] = timed(lambda rep: [(1, (3 + rep) % n_slots, fi + 4 + rep, fe.BOW_QUERY | fe.BOW_ADD)])
    gather_bytes = n_db * n_desc * L * k * 32
    walk = [x[0] for x in res["batch_query_add"]["device_ms_per_launch"]]
    res["walk_kernel"] = dict(bytes_gathered=gather_bytes, ms_min_max=[min(walk), max(walk)], TB_per_s_min_max=[gather_bytes / max(walk) / 1e9, gather_bytes / min(walk) / 1e9],
                              infinity_cache_gather_TB_per_s=8.6,
                              note="bytes = descriptors x levels x k x 32 B (sibling groups fetched); the guide's 8.6 TB/s is whole rows of a 38 MB table gathered at random")
    if handle is None:
        h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    r = run(a.rehearse)
    print(json.dumps(r, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
