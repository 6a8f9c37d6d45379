"""vg_voc_load / vg_bow_* / vg_kf_loop_detect (include/vinsgpu.h): DBoW2 loop detection as PoseGraph::detectLoop uses it.  DBoW2 is vendored
in the reference (pose_graph/src/ThirdParty/DBoW, VocabularyBinary.*) and was READ there; this file restates the five definitions of the
header (vocabulary, word of a descriptor, BoW vector, query, decision) in plain Python float64 with none of the kernels' shortcuts (no
renumbering, no sort, no lane groups: dictionaries and loops), and holds the synthetic vocabularies, the scenes, the conditions the scenes
must meet (asserted on the CPU by the restatement alone: test_scene_conditions of tests/test_kf_bow_simt.py) and the check bodies shared by
tests/test_kf_bow_simt.py (the emulated kernels) and tests/test_kf_bow_gpu.py (the MI355X).

Nothing in the definition multiplies and adds in one expression: additions, fabs, one division per word, one halving.  Every quantity is
therefore compared for EQUALITY, doubles by their bit patterns."""
import functools
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY, ADD = 1, 2
STOPPED = 0xFFFFFFFF
BAD_ARG = -1
VOC_NODE = np.dtype([("node_id", "<i4"), ("parent_id", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])
VOC_WORD = np.dtype([("node_id", "<i4"), ("word_id", "<i4")])


def _fe():
    import __graft_entry__ as graft
    graft.load_package()
    from vins_mono_amd import fe
    return fe


# --------------------------------------------------------------------------------------------------- the restatement
def as_int(d):
    """a descriptor (4 little-endian 64-bit words, bit i in word i / 64 at position i % 64) as one 256-bit integer"""
    return int(d[0]) | int(d[1]) << 64 | int(d[2]) << 128 | int(d[3]) << 192


def as_words(x):
    return [(x >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]


def popcount(x):
    return bin(x).count("1")


class Voc:
    """TemplatedVocabulary::loadBin: the children of a node are the records naming it as parent, in record order"""

    def __init__(self, k, L, nodes, words):
        self.k, self.L, self.nodes, self.words = k, L, nodes, words
        self.children, self.desc, self.weight, self.word_id = {0: []}, {}, {}, {}
        for r in nodes:
            nid, pid = int(r["node_id"]), int(r["parent_id"])
            self.children.setdefault(nid, [])
            self.children.setdefault(pid, []).append(nid)
            self.desc[nid], self.weight[nid] = as_int(r["descriptor"]), float(r["weight"])
        for r in words:
            self.word_id[int(r["node_id"])] = int(r["word_id"])

    def transform(self, d, last_wins=False):
        """(word id, weight) of the 256-bit integer d: transform:1217-1258; the update is on d < best_d only, so the first child wins a tie"""
        node = 0
        while self.children[node]:
            best, best_d = None, None
            for c in self.children[node]:
                dist = popcount(d ^ self.desc[c])
                if best is None or dist < best_d or (last_wins and dist == best_d):
                    best, best_d = c, dist
            node = best
        return self.word_id[node], self.weight[node]

    def word_of_keypoint(self, descs):
        out = np.zeros(len(descs), np.uint32)
        for i, d in enumerate(descs):
            w, wt = self.transform(as_int(d))
            out[i] = w if wt > 0 else STOPPED
        return out

    def bow(self, descs):
        """transform:1065-1121 with BowVector::addWeight and normalize (L1): ([word ids ascending], [values])"""
        v = {}
        for d in descs:
            w, wt = self.transform(as_int(d))
            if wt > 0:
                if w in v:
                    v[w] += wt
                else:
                    v[w] = wt
        ws = sorted(v)
        norm = 0.0
        for w in ws:
            norm += abs(v[w])
        if norm > 0.0:
            for w in ws:
                v[w] /= norm
        return np.array(ws, np.uint32), np.array([v[w] for w in ws], np.float64)


class Db:
    """TemplatedDatabase with the inverted file, queryL1 and PoseGraph::detectLoop's decision"""

    def __init__(self):
        self.entries, self.ifile = [], {}

    def query(self, vec, frame_index, all_pairs=False):
        ws, vs = vec
        max_id, n = frame_index - 50, len(self.entries)
        pairs = {}
        for w, q in zip(ws.tolist(), vs.tolist()):
            for e, d in self.ifile.get(w, []):
                if e < max_id or max_id == -1 or e == n - 1:
                    value = abs(q - d) - abs(q) - abs(d)
                    if e in pairs:
                        pairs[e] += value
                    else:
                        pairs[e] = value
        ret = sorted((v, e) for e, v in pairs.items())
        if all_pairs:
            return ret
        return [(e, -v / 2.0) for v, e in ret[:4]]

    def add(self, vec):
        e = len(self.entries)
        self.entries.append(vec)
        for w, d in zip(vec[0].tolist(), vec[1].tolist()):
            self.ifile.setdefault(w, []).append((e, d))
        return e

    def detect(self, vec, frame_index, flags=QUERY | ADD):
        ret = self.query(vec, frame_index) if flags & QUERY else []
        entry = self.add(vec) if flags & ADD else -1
        find_loop = False
        if len(ret) >= 1 and ret[0][1] > 0.05:
            for i in range(1, len(ret)):
                if ret[i][1] > 0.015:
                    find_loop = True
        loop_index = -1
        if find_loop and frame_index > 50:
            min_index = -1
            for i in range(len(ret)):
                if min_index == -1 or (ret[i][0] < min_index and ret[i][1] > 0.015):
                    min_index = ret[i][0]
            loop_index = min_index
        return dict(entry_id=entry, n_results=len(ret), ids=np.array([e for e, _ in ret], np.int32), scores=np.array([s for _, s in ret], np.float64),
                    find_loop=int(find_loop), loop_index=loop_index, n_words=len(vec[0]))


# --------------------------------------------------------------------------------------------------- the synthetic vocabularies
def rnd_desc(rng, n):
    return rng.integers(0, 2 ** 63, (n, 4), dtype=np.int64).astype(np.uint64) ^ (rng.integers(0, 2, (n, 4), dtype=np.int64).astype(np.uint64) << np.uint64(63))


def flip(desc, bits):
    d = np.array(desc, np.uint64).copy()
    for b in bits:
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


NONUNIFORM = [[["L", "L", "L"]], "L", [["L", "L"], "L", ["L", "L", "L", "L"]], ["L", "L"], "L"]     # a node with one child; a leaf at depth 1 beside leaves at depth 3
VOCS = {"k3L2": (3, 2, 11), "k10L3": (10, 3, 12), "k10L4": (10, 4, 13), "k17L2": (17, 2, 14), "nonuniform": (5, 3, 15)}


def _shape(name):
    k, L, _ = VOCS[name]
    if name == "nonuniform":
        return NONUNIFORM
    t = "L"
    for _ in range(L):
        t = [t] * k
    return t


def probes(name):
    """two fixed descriptors whose words get weight 0 and -1: the stopped words every vocabulary has"""
    return rnd_desc(np.random.default_rng(1000 + VOCS[name][2]), 2)


@functools.lru_cache(maxsize=None)
def voc(name):
    """random descriptors, positive random weights on the leaves, word ids in a random order; in `nonuniform` the node ids are a random
    permutation and the records are shuffled, so that child order differs from id order"""
    k, L, seed = VOCS[name]
    rng = np.random.default_rng(seed)
    recs, leaves = [], []

    def walk(t, parent):
        for c in t:
            nid = len(recs) + 1
            recs.append([nid, parent])
            if c == "L":
                leaves.append(nid)
            else:
                walk(c, nid)

    walk(_shape(name), 0)
    n = len(recs)
    perm = np.arange(1, n + 1)
    order = np.arange(n)
    if name == "nonuniform":
        perm, order = rng.permutation(n) + 1, rng.permutation(n)
    ren = lambda v: 0 if v == 0 else int(perm[v - 1])
    nodes = np.zeros(n, VOC_NODE)
    desc = rnd_desc(rng, n)
    is_leaf = set(leaves)
    for j, i in enumerate(order):
        nid, pid = recs[i]
        nodes[j] = (ren(nid), ren(pid), float(rng.uniform(0.5, 9.0)) if nid in is_leaf else 0.0, desc[i])
    words = np.zeros(len(leaves), VOC_WORD)
    wid = rng.permutation(len(leaves))
    for j, nid in enumerate(leaves):
        words[j] = (ren(nid), int(wid[j]))
    v = Voc(k, L, nodes, words)
    if name == "nonuniform":
        kids = v.children[0]
        assert [c for c in kids] != sorted(kids), "child order equals id order"
        assert any(len(v.children[c]) == 1 for c in kids) and any(not v.children[c] for c in kids)
    kids = v.children[0]
    for fix, other in ((kids[0], kids[1]), (kids[-1], kids[-2])):                  # an even distance, so that a descriptor can tie between them
        if popcount(v.desc[fix] ^ v.desc[other]) % 2:
            nodes["descriptor"][np.flatnonzero(nodes["node_id"] == fix)[0], 0] ^= np.uint64(1)
    v = Voc(k, L, nodes, words)
    # the stopped words: where the two probes land
    stop = [v.transform(as_int(p))[0] for p in probes(name)]
    assert stop[0] != stop[1]
    node_of = {int(r["word_id"]): int(r["node_id"]) for r in words}
    for w, wt in zip(stop, (0.0, -1.0)):
        nodes["weight"][nodes["node_id"] == node_of[w]] = wt
    return Voc(k, L, nodes, words)


def tie_descriptor(v, node, a, b):
    """a descriptor equidistant from children a and b (positions) of `node`, closer to both than to any other child (the two are an even
    distance apart: voc() sees to that for the root's first and last pair)"""
    kids = v.children[node]
    ca, cb = v.desc[kids[a]], v.desc[kids[b]]
    diff = [i for i in range(256) if (ca ^ cb) >> i & 1]
    assert len(diff) % 2 == 0
    d = ca
    for i in diff[:len(diff) // 2]:
        d ^= 1 << i
    da = popcount(d ^ ca)
    assert da == popcount(d ^ cb) and all(popcount(d ^ v.desc[c]) > da for i, c in enumerate(kids) if i not in (a, b)), "the tie is not the minimum"
    return np.array(as_words(d), np.uint64)


@functools.lru_cache(maxsize=None)
def walk_record(name, n):
    """n descriptors: the planted ones first (as many as fit), then random ones"""
    v = voc(name)
    kids = v.children[0]
    planted = [tie_descriptor(v, 0, len(kids) - 2, len(kids) - 1)]                     # (children 15 and 16 of the 17-child root)
    planted.append(np.array(as_words(v.desc[kids[len(kids) // 2]]), np.uint64))        # equal to a node's
    planted.append(np.zeros(4, np.uint64))
    planted.append(np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64))
    planted.extend(probes(name))                                                       # land on the stopped words
    planted.append(tie_descriptor(v, 0, 0, 1))
    first = v.transform(as_int(planted[0]))[0]
    assert first != v.transform(as_int(planted[0]), last_wins=True)[0], "first-wins and last-wins give the same word"
    out = np.concatenate([np.array(planted, np.uint64), rnd_desc(np.random.default_rng(77 + n), max(n, 1))])[:n]
    return out


WALK_SIZES = (1, 63, 64, 65)
WALK_LARGE = (5000, 9000)           # (9000: beyond the word ids a workgroup sorts in LDS)


@functools.lru_cache(maxsize=None)
def repeat_record(name="k10L3"):
    """one word 1, 2, 3, 4, 7 and 64 times, the rest once; for the word seen 7 times the repeated sum differs from 7 * w"""
    v = voc(name)
    rng = np.random.default_rng(5)
    cand = rnd_desc(rng, 400)
    seen, picks = set(), []
    for d in cand:
        w, wt = v.transform(as_int(d))
        if wt > 0 and w not in seen:
            seen.add(w)
            picks.append((d, wt))
    seven = None
    for i, (d, wt) in enumerate(picks):
        s = wt
        for _ in range(6):
            s += wt
        if s != 7 * wt:
            seven = i
            break
    assert seven is not None, "no weight whose repeated sum differs from 7 * w"
    d7 = picks.pop(seven)[0]
    counts = [(picks[0][0], 1), (picks[1][0], 2), (picks[2][0], 3), (picks[3][0], 4), (d7, 7), (picks[4][0], 64)]
    rows = [d for d, c in counts for _ in range(c)] + [p[0] for p in picks[5:25]]
    rows = np.array(rows, np.uint64)
    return rows[rng.permutation(len(rows))]


def vector_records(name="k10L3"):
    return {"repeats": repeat_record(name), "only_stopped": np.array([probes(name)[i % 2] for i in range(5)], np.uint64), "empty": np.zeros((0, 4), np.uint64)}


# --------------------------------------------------------------------------------------------------- the stream
STREAM_VOC = "k10L4"
N_STREAM = 70
STREAM_SEED = 22        # (a seed under which the stream meets every condition of stream_reference: most do not, by a tie or a missing kind)
REVISITS = {52: 1, 60: 5, 65: 10}


@functools.lru_cache(maxsize=None)
def stream():
    """70 keyframes of 40 - 200 descriptors.  A frame shares about half its descriptors (a few bits flipped) with the one before it, as
    consecutive keyframes do; frames 0, 1, 2, 10 and 11 start afresh (frames 0, 1 and 10 stand alone); frame 52 revisits frame 1, frame 60
    frame 5, frame 65 frame 10."""
    rng = np.random.default_rng(STREAM_SEED)
    frames = []
    noisy = lambda ds: np.array([flip(d, rng.integers(0, 256, int(rng.integers(0, 3)))) for d in ds], np.uint64).reshape(-1, 4)
    for f in range(N_STREAM):
        n = int(rng.integers(40, 201))
        if f in (0, 1, 2, 10, 11):
            d = rnd_desc(rng, n)
        else:
            prev = frames[-1]
            take = prev[rng.permutation(len(prev))[:min(len(prev), n) // 2]]
            if f in REVISITS:
                old = frames[REVISITS[f]]
                d = np.concatenate([noisy(old), noisy(take[:20])])
            else:
                d = np.concatenate([noisy(take), rnd_desc(rng, n - len(take))])
            d = d[rng.permutation(len(d))][:200]
        frames.append(d)
    assert all(40 <= len(d) <= 200 for d in frames)
    return frames


@functools.lru_cache(maxsize=None)
def stream_vectors():
    v = voc(STREAM_VOC)
    return [v.bow(d) for d in stream()]


@functools.lru_cache(maxsize=None)
def stream_reference():
    """detectLoop over the stream on one database; the conditions the scene must meet, and the tie condition, asserted here"""
    db, out, kinds = Db(), [], set()
    for f, vec in enumerate(stream_vectors()):
        allp = db.query(vec, f, all_pairs=True)
        top = [v for v, _ in allp[:5]]
        assert len(set(top)) == len(top), ("the tie condition: two of the 4 kept values and the best rejected one are equal", f, top)
        r = db.detect(vec, f)
        out.append(r)
        if r["find_loop"] and r["loop_index"] >= 0:
            kinds.add("loop")
        if r["find_loop"] and f <= 50:
            kinds.add("gated")
        if r["n_results"] and r["ids"][0] == f - 1:
            kinds.add("previous_first")
        if 0 < r["n_results"] < 4:
            kinds.add("fewer_than_4")
        if r["n_results"] == 0:
            kinds.add("none")
        if r["loop_index"] >= 0 and r["loop_index"] == r["ids"][0] and any(i < r["ids"][0] and s <= 0.015 for i, s in zip(r["ids"][1:], r["scores"][1:])):
            kinds.add("id0_kept")
    missing = {"loop", "gated", "previous_first", "fewer_than_4", "none", "id0_kept"} - kinds
    assert not missing, missing
    return out


def check_scene_conditions():
    """CPU only: what the restatement asserts about its own scenes"""
    for name in VOCS:
        voc(name)
        for n in WALK_SIZES:
            walk_record(name, n)
    repeat_record()
    ref = stream_reference()
    assert ref[52]["loop_index"] == 1 and ref[60]["loop_index"] >= 0 and ref[65]["ids"][0] == 10


# --------------------------------------------------------------------------------------------------- the device checks
# one body for the emulator and the MI355X; h: a ba.Handle
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def setup(h, name, max_keypoints, n_slots, n_db, max_entries, pool_words, load=True):
    """keyframe records (descriptors are planted with vg_kf_set), the vocabulary, the databases"""
    fe = _fe()
    import kf_brief_ref as KB
    kf = fe.KeyFrames(h, 67, 41, max_keypoints, 8, n_slots, KB.pattern())
    if load:
        v = voc(name)
        fe.voc_load(h, v.k, v.L, v.nodes, v.words)
    fe.bow_configure(h, n_db, max_entries, pool_words)
    return kf


def plant(kf, slot, descs):
    n = len(descs)
    kf.set(slot, np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros((n, 2), np.float32), descs, np.zeros((0, 2), np.float32), np.zeros((0, 4), np.uint64))


def same_result(g, r, what):
    for k in ("entry_id", "n_results", "find_loop", "loop_index", "n_words"):
        assert g[k] == r[k], (what, k, g[k], r[k])
    assert np.array_equal(g["ids"], r["ids"]), (what, g["ids"], r["ids"])
    assert np.array_equal(bits(g["scores"]), bits(r["scores"])), (what, g["scores"], r["scores"])


def same_dict(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a if k != "device_ms") and set(a) == set(b)


def check_walk(h, name, sizes):
    """word_of_keypoint of every descriptor, the vector (word ids, value bit patterns, n_words)"""
    fe = _fe()
    v = voc(name)
    cap = max(sizes)
    kf = setup(h, name, cap, 1, 1, 2, cap)
    for n in sizes:
        d = walk_record(name, n)
        plant(kf, 0, d)
        g = fe.kf_loop_detect(h, [(0, 0, 0, QUERY)], taps=cap)[0]
        want = v.word_of_keypoint(d)
        assert np.array_equal(g["word_of_keypoint"][:n], want), (name, n, np.flatnonzero(g["word_of_keypoint"][:n] != want)[:8])
        assert (g["word_of_keypoint"][n:] == 0xDEADBEEF).all(), (name, n, "written beyond the record's count")
        ws, vs = v.bow(d)
        assert g["n_words"] == len(ws) and np.array_equal(g["bow_word"], ws) and np.array_equal(bits(g["bow_value"]), bits(vs)), (name, n)
        assert g["n_results"] == 0 and g["entry_id"] == -1 and fe.bow_count(h, 0) == (0, 0)
        if n >= 7:
            assert (want[4:6] == STOPPED).all()
    print(f"kf_bow walk {name}: records of {sizes} equal")


def check_vector(h, name="k10L3"):
    fe = _fe()
    v = voc(name)
    kf = setup(h, name, 256, 1, 1, 4, 512)
    for what, d in vector_records(name).items():
        plant(kf, 0, d)
        g = fe.kf_loop_detect(h, [(0, 0, 49, QUERY | ADD)], taps=256)[0]
        ws, vs = v.bow(d)
        assert g["n_words"] == len(ws) and np.array_equal(g["bow_word"], ws) and np.array_equal(bits(g["bow_value"]), bits(vs)), what
        assert np.array_equal(g["word_of_keypoint"][:len(d)], v.word_of_keypoint(d)), what
        assert not np.isnan(g["bow_value"]).any()
        if what != "repeats":
            assert g["n_words"] == 0 and g["n_results"] == 0
    assert fe.bow_count(h, 0)[0] == 3
    w, x = fe.bow_get(h, 0, 2)
    assert len(w) == 0 and len(x) == 0


def check_stream(h):
    """the 70 keyframes on one database, detectLoop frame by frame"""
    fe = _fe()
    ref, frames = stream_reference(), stream()
    kf = setup(h, STREAM_VOC, 200, 2, 1, N_STREAM, 200 * N_STREAM)
    loops = 0
    for f, d in enumerate(frames):
        plant(kf, f % 2, d)
        g = fe.kf_loop_detect(h, [(0, f % 2, f, QUERY | ADD)])[0]
        same_result(g, ref[f], ("stream", f))
        loops += g["loop_index"] >= 0
    vecs = stream_vectors()
    assert fe.bow_count(h, 0) == (N_STREAM, sum(len(v[0]) for v in vecs))
    for e in (0, 33, 69):
        w, x = fe.bow_get(h, 0, e)
        assert np.array_equal(w, vecs[e][0]) and np.array_equal(bits(x), bits(vecs[e][1])), e
    print(f"kf_bow stream: 70 frames equal, {loops} loops returned")


def check_tie(h):
    """two identical entries: the library's own rule, ascending entry id"""
    fe = _fe()
    frames = stream()
    kf = setup(h, STREAM_VOC, 200, 2, 1, 4, 1000)
    plant(kf, 0, frames[5])
    plant(kf, 1, frames[60])
    for _ in range(2):
        fe.kf_loop_detect(h, [(0, 0, 0, ADD)])
    g = fe.kf_loop_detect(h, [(0, 1, 49, QUERY)])[0]
    assert list(g["ids"]) == [0, 1] and bits(g["scores"])[0] == bits(g["scores"])[1] and g["scores"][0] > 0.05, g


def check_flags_and_state(h):
    fe = _fe()
    frames, vecs = stream()[3:], stream_vectors()[3:]                              # (three consecutive keyframes that share descriptors)
    v = voc(STREAM_VOC)
    kf = setup(h, STREAM_VOC, 200, 3, 2, 8, 2000)
    for s in range(3):
        plant(kf, s, frames[s])
    ref = Db()
    # ADD only: addKeyFrameIntoVoc
    for s in range(2):
        g = fe.kf_loop_detect(h, [(0, s, 0, ADD)], taps=200)[0]
        same_result(g, ref.detect(vecs[s], 0, ADD), ("add only", s))
        w, x = fe.bow_get(h, 0, s)
        assert np.array_equal(w, g["bow_word"]) and np.array_equal(bits(x), bits(g["bow_value"])), "vg_bow_get against the tap of the call that added it"
    # QUERY only: nothing is added
    before = fe.bow_count(h, 0)
    g = fe.kf_loop_detect(h, [(0, 2, 49, QUERY)])[0]
    same_result(g, ref.detect(vecs[2], 49, QUERY), "query only")
    assert g["n_results"] == 2 and fe.bow_count(h, 0) == before == (2, len(vecs[0][0]) + len(vecs[1][0]))
    # reset
    assert fe.bow_count(h, 1) == (0, 0)
    fe.bow_reset(h, 0)
    assert fe.bow_count(h, 0) == (0, 0)
    g = fe.kf_loop_detect(h, [(0, 2, 49, QUERY | ADD)])[0]
    same_result(g, Db().detect(vecs[2], 49), "after reset")
    # the vocabulary again: every database is empty
    fe.kf_loop_detect(h, [(1, 0, 0, ADD)])
    assert fe.bow_count(h, 0)[0] == 1 and fe.bow_count(h, 1)[0] == 1
    fe.voc_load(h, v.k, v.L, v.nodes, v.words)
    assert fe.bow_count(h, 0) == (0, 0) and fe.bow_count(h, 1) == (0, 0)
    g = fe.kf_loop_detect(h, [(0, 2, 49, QUERY | ADD)])[0]
    same_result(g, Db().detect(vecs[2], 49), "after the second vg_voc_load")


def check_batches(h, sizes=(1, 3, 33)):
    """33 databases with different histories: a batch equals the single calls bit for bit; two databases fed the same stream stay identical"""
    fe = _fe()
    frames, vecs = stream(), stream_vectors()
    ND = 33
    kf = setup(h, STREAM_VOC, 200, 40, ND + 2, 12, 2400)
    for s in range(40):
        plant(kf, s, frames[s])
    hist = [1 + (i * 7) % 6 for i in range(ND)]
    hist[4] = 0
    refs = [Db() for _ in range(ND)]
    for j in range(max(hist)):
        reqs = [(i, (i + j) % 40, 0, ADD) for i in range(ND) if j < hist[i]]
        fe.kf_loop_detect(h, reqs)
        for i, s, _, _ in reqs:
            refs[i].add(vecs[s])
    for n in sizes:
        reqs = [(i, (2 * i + 1) % 40, 49, QUERY) for i in range(n)]
        together = fe.kf_loop_detect(h, reqs, taps=200)
        for i, rq in enumerate(reqs):
            alone = fe.kf_loop_detect(h, [rq], taps=200)[0]
            assert same_dict(together[i], alone), (n, i)
            same_result(alone, refs[i].detect(vecs[rq[1]], 49, QUERY), ("batch", n, i))
    assert len({g["n_results"] for g in together}) >= 3
    reqs = [(i, (2 * i + 1) % 40, 49, QUERY | ADD) for i in range(ND)]
    together = fe.kf_loop_detect(h, reqs)
    for i, rq in enumerate(reqs):
        same_result(together[i], refs[i].detect(vecs[rq[1]], 49), ("batch add", i))
        assert fe.bow_count(h, i) == (hist[i] + 1, sum(len(e[0]) for e in refs[i].entries))
    # two databases, the same stream, side by side in every call
    a, b = ND, ND + 1
    for f in range(8):
        g = fe.kf_loop_detect(h, [(a, f, 49, QUERY | ADD), (b, f, 49, QUERY | ADD)])
        assert same_dict(g[0], g[1]), f
    for e in range(8):
        (w0, x0), (w1, x1) = fe.bow_get(h, a, e), fe.bow_get(h, b, e)
        assert np.array_equal(w0, w1) and np.array_equal(bits(x0), bits(x1))


# ---- refusals
def _voc_refusals():
    """name -> (nodes, words, scoring, weighting) of a small vocabulary spoiled in one way"""
    v = voc("k3L2")
    out = {}

    def case(name, edit=None, scoring=0, weighting=0):
        nodes, words = v.nodes.copy(), v.words.copy()
        if edit:
            nodes, words = edit(nodes, words) or (nodes, words)
        out[name] = (nodes, words, scoring, weighting)

    inner = int(v.children[0][0])
    leaf = int(v.words["node_id"][0])

    def set_node(field, idx, val):
        def f(n, w):
            n[field][idx] = val
        return f

    def set_word(field, idx, val):
        def f(n, w):
            w[field][idx] = val
        return f

    case("node_id_0", set_node("node_id", 2, 0))
    case("node_id_beyond", set_node("node_id", 2, len(v.nodes) + 1))
    case("node_id_repeated", set_node("node_id", 2, int(v.nodes["node_id"][3])))
    case("parent_beyond", set_node("parent_id", 2, len(v.nodes) + 1))
    case("parent_negative", set_node("parent_id", 2, -1))
    i_in = int(np.flatnonzero(v.nodes["node_id"] == inner)[0])
    case("unreachable", set_node("parent_id", i_in, inner))                       # a node that is its own parent: its subtree hangs in the air
    case("word_on_inner_node", set_word("node_id", 0, inner))
    case("leaf_without_word", set_word("node_id", 0, int(v.words["node_id"][1])))
    case("word_id_beyond", set_word("word_id", 0, len(v.words)))
    case("word_id_negative", set_word("word_id", 0, -1))
    case("word_id_repeated", set_word("word_id", 0, int(v.words["word_id"][1])))

    def empty_root(n, w):
        n["parent_id"][n["parent_id"] == 0] = inner
    case("empty_root", empty_root)
    case("scoring_l2", None, scoring=1)
    case("weighting_tf", None, weighting=1)
    return out


VOC_REFUSALS = tuple(_voc_refusals())
CALL_REFUSALS = ("no_vocabulary", "no_bow_configure", "no_kf_configure", "in_struct_size", "out_struct_size", "db_beyond", "db_negative", "slot_beyond",
                 "slot_never_filled", "same_db_twice", "flags_0", "flags_4", "database_full", "pool_short")


def _good_state(h):
    """one database with two entries, a third record ready: (kf, the reference's answer for the next detectLoop)"""
    fe = _fe()
    frames, vecs = stream(), stream_vectors()
    kf = setup(h, STREAM_VOC, 200, 4, 2, 3, len(vecs[0][0]) + len(vecs[1][0]) + len(frames[2]))
    ref = Db()
    for s in range(3):
        plant(kf, s, frames[s])
    for s in range(2):
        fe.kf_loop_detect(h, [(0, s, 0, ADD)])
        ref.add(vecs[s])
    return kf, ref


def check_voc_refusal(h, name):
    """refused with VG_ERR_BAD_ARG, the loaded vocabulary and the databases as they were: the next good call gives the reference's result"""
    fe = _fe()
    kf, ref = _good_state(h)
    before = fe.bow_count(h, 0)
    nodes, words, scoring, weighting = _voc_refusals()[name]
    rc = fe._bow_lib(h).vg_voc_load(h.h, 3, 2, scoring, weighting, len(nodes), nodes.ctypes.data, len(words), words.ctypes.data)
    assert rc == BAD_ARG, (name, rc)
    assert fe.bow_count(h, 0) == before
    same_result(fe.kf_loop_detect(h, [(0, 2, 49, QUERY | ADD)])[0], ref.detect(stream_vectors()[2], 49), name)


def check_call_refusal(h, name, new_handle):
    fe = _fe()
    C = fe.C
    vecs = stream_vectors()
    if name in ("no_vocabulary", "no_bow_configure", "no_kf_configure"):
        import kf_brief_ref as KB
        h2 = new_handle()
        try:
            v = voc("k3L2")
            if name != "no_kf_configure":
                fe.KeyFrames(h2, 67, 41, 16, 8, 1, KB.pattern())
            if name != "no_vocabulary":
                fe.voc_load(h2, v.k, v.L, v.nodes, v.words)
            if name == "no_vocabulary":
                assert fe._bow_lib(h2).vg_bow_configure(h2.h, 1, 4, 64) == BAD_ARG
            if name == "no_kf_configure":
                fe.bow_configure(h2, 1, 4, 64)
            a, o = fe.BowIn(), fe.BowOut()
            a.struct_size, a.flags, o.struct_size, o.entry_id = C.sizeof(fe.BowIn), QUERY, C.sizeof(fe.BowOut), -7
            assert fe._bow_lib(h2).vg_kf_loop_detect(h2.h, 1, C.byref(a), C.byref(o)) == BAD_ARG and o.entry_id == -7, name
        finally:
            h2.close()
        return
    kf, ref = _good_state(h)
    if name == "database_full":
        fe.kf_loop_detect(h, [(0, 2, 0, ADD)])
        ref.add(vecs[2])
    if name == "pool_short":
        plant(kf, 3, np.concatenate([stream()[2], stream()[3][:1]]))              # one keypoint more than the pool has room for
    before = [fe.bow_count(h, d) for d in (0, 1)]
    ins, outs = (fe.BowIn * 2)(), (fe.BowOut * 2)()
    for i, (db, slot) in enumerate(((1, 0), (0, 2))):                              # a good neighbour in front of the bad request
        ins[i].struct_size, ins[i].db, ins[i].slot, ins[i].frame_index, ins[i].flags = C.sizeof(fe.BowIn), db, slot, 49, QUERY | ADD
        outs[i].struct_size, outs[i].entry_id, outs[i].n_results, outs[i].loop_index = C.sizeof(fe.BowOut), -7, -8, -9
    bad = ins[1]
    if name == "in_struct_size":
        bad.struct_size = 8
    elif name == "out_struct_size":
        outs[1].struct_size = 8
    elif name == "db_beyond":
        bad.db = 2
    elif name == "db_negative":
        bad.db = -1
    elif name == "slot_beyond":
        bad.slot = 4
    elif name == "slot_never_filled":
        import kf_brief_ref as KB
        kf.configure(67, 41, 200, 8, 4, KB.pattern())                              # (fresh records: none filled)
        for s in range(3):
            plant(kf, s, stream()[s])
        bad.slot = 3
    elif name == "same_db_twice":
        bad.db = 1
    elif name == "flags_0":
        bad.flags = 0
    elif name == "flags_4":
        bad.flags = 4 | QUERY
    elif name == "pool_short":
        bad.slot = 3
    rc = h.lib.vg_kf_loop_detect(h.h, 2, ins, outs)
    assert rc == BAD_ARG, (name, rc)
    for i in range(2):
        assert (outs[i].entry_id, outs[i].n_results, outs[i].loop_index) == (-7, -8, -9), (name, i)
    assert [fe.bow_count(h, d) for d in (0, 1)] == before, name
    if name == "database_full":
        same_result(fe.kf_loop_detect(h, [(0, 2, 49, QUERY)])[0], ref.detect(vecs[2], 49, QUERY), name)
    else:
        same_result(fe.kf_loop_detect(h, [(0, 2, 49, QUERY | ADD)])[0], ref.detect(vecs[2], 49), name)


# ---- the chain
def check_chain(h, size=(100, 70)):
    """vg_kf_add of a revisited frame -> vg_kf_loop_detect returns the first visit's entry -> that slot into vg_kf_match: the match list is
    the one obtained by naming the slot directly.  Entry e of the database is the keyframe in slot e."""
    import kf_brief_ref as KB
    fe = _fe()
    v = voc("k10L3")
    f0, f1 = KB.frames(size)
    cam = KB.camera_struct(KB.cameras(size[0])["pinhole"])
    none = np.zeros((0, 2), np.float32)
    NS = 58
    kf = fe.KeyFrames(h, size[0], size[1], 150, 150, NS, KB.pattern())
    fe.voc_load(h, v.k, v.L, v.nodes, v.words)
    fe.bow_configure(h, 1, NS, 150 * NS)
    first = kf.add([0, 1], [f1, f0], [cam, cam], [none, none])                     # entry 0: the frame that will be revisited
    ref, rng = Db(), np.random.default_rng(3)
    descs = [first[0]["descriptors"], first[1]["descriptors"]]
    for s in range(2, 56):                                                         # the way round: keyframes that look like nothing else
        descs.append(rnd_desc(rng, 60))
        n = len(descs[-1])
        kf.set(s, np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros((n, 2), np.float32), descs[-1], none, np.zeros((0, 4), np.uint64))
    for s in range(56):
        g = fe.kf_loop_detect(h, [(0, s, s, QUERY | ADD)])[0]
        same_result(g, ref.detect(v.bow(descs[s]), s), ("chain", s))
    # the revisit: the same image again, its own corners as window points
    kf.add([56], [f1], [cam], [first[0]["keypoints"][:150]], arrays=False)
    g = fe.kf_loop_detect(h, [(0, 56, 56, QUERY | ADD)])[0]
    want = ref.detect(v.bow(descs[0]), 56)
    same_result(g, want, "the revisit")
    assert g["find_loop"] == 1 and g["loop_index"] == 0 == g["ids"][0], g
    old = g["loop_index"]                                                          # entry id = slot
    m_loop, m_named = kf.match([(56, old)])[0], kf.match([(56, 0)])[0]
    assert same_dict(m_loop, m_named) and m_loop["n_matched"] > KB.MIN_LOOP_NUM
    print(f"kf_bow chain: the revisit scores {g['scores'][:2]} against entries {g['ids'][:2]}; loop_index {old}; {m_loop['n_matched']} matches")


# --------------------------------------------------------------------------------------------------- the host tools' files
def write_voc_bin(path, v, scoring=0, weighting=0):
    """the reference's .bin layout: 6 x int32 header, the node records, the word records"""
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", v.k, v.L, scoring, weighting, len(v.nodes), len(v.words)))
        f.write(np.ascontiguousarray(v.nodes, VOC_NODE).tobytes())
        f.write(np.ascontiguousarray(v.words, VOC_WORD).tobytes())


def write_frames(path, frames, first_index=0):
    """BOW1: magic, n_frames, first frame_index | per frame: n, descriptors"""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", 0x31574F42, len(frames), first_index))
        for d in frames:
            f.write(struct.pack("<i", len(d)))
            f.write(np.ascontiguousarray(d, "<u8").tobytes())


REPLAY_CASES = {"stream_head": ("k10L4", 0, 12, 0), "around_50": ("k10L4", 0, 62, 0), "nonuniform": ("nonuniform", None, 6, 47)}


def replay_frames(name):
    vname, lo, n, first = REPLAY_CASES[name]
    if lo is None:
        return vname, [walk_record(vname, m) for m in (63, 64, 65, 1, 63, 64)], first
    return vname, stream()[lo:lo + n], first


def binding_lines(h, name):
    """what `vins_replay bow` must print, from the binding on the same input"""
    fe = _fe()
    vname, frames, first = replay_frames(name)
    kf = setup(h, vname, 200, 1, 1, len(frames), 200 * len(frames))
    lines = []
    for i, d in enumerate(frames):
        plant(kf, 0, d)
        g = fe.kf_loop_detect(h, [(0, 0, first + i, QUERY | ADD)])[0]
        lines.append(result_line(first + i, g))
    return lines


def result_line(frame_index, g):
    return " ".join([str(frame_index), str(g["loop_index"]), str(g["find_loop"]), str(g["entry_id"]), str(g["n_words"]), str(g["n_results"])] +
                    [f"{int(i)}:{int(s):016x}" for i, s in zip(g["ids"], bits(g["scores"]))])


def check_replay(h, exe, tmp_dir, name):
    """`vins_replay bow` (BriefVocabulary, PoseGraph::loadVocabulary / detectLoop over KeyFrame's slot, vg_pack_bow) against the binding"""
    vname, frames, first = replay_frames(name)
    vb, src, dst = (os.path.join(str(tmp_dir), name + e) for e in (".voc.bin", ".frames.bin", ".txt"))
    write_voc_bin(vb, voc(vname))
    write_frames(src, frames, first)
    r = subprocess.run([exe, "bow", vb, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(dst).read().splitlines() == binding_lines(h, name), name


def check_voc_file(h, tmp_dir):
    """read_voc_bin of a file in the record layout equals the arrays it was written from, and the load of it gives the same words"""
    fe = _fe()
    v = voc("nonuniform")
    p = os.path.join(str(tmp_dir), "voc.bin")
    write_voc_bin(p, v)
    k, L, sc, wt, nodes, words = fe.read_voc_bin(p)
    assert (k, L, sc, wt) == (v.k, v.L, 0, 0) and nodes.tobytes() == v.nodes.tobytes() and words.tobytes() == v.words.tobytes()
    kf = setup(h, "nonuniform", 65, 1, 1, 2, 65)
    d = walk_record("nonuniform", 65)
    plant(kf, 0, d)
    a = fe.kf_loop_detect(h, [(0, 0, 0, QUERY)], taps=65)[0]
    fe.voc_load(h, k, L, nodes, words)
    b = fe.kf_loop_detect(h, [(0, 0, 0, QUERY)], taps=65)[0]
    assert same_dict(a, b)
