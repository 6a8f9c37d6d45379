"""vg_vio_* (the front end feeds the resident sequences on the device: one call per frame) against the path a caller had before it, run on
a SECOND handle from the same seeded state: every frame through vg_fe_tracks_step, its msg_id / msg_obs pointers handed to
vg_ba_seq_step_imu_async with the same samples.  Both paths run the same kernels on the same bits, so every comparison is exact: ints
equal, floats and doubles by bit pattern.  No tolerance anywhere in this file.

Used by tests/test_vio_bridge.py under the emulator (`not gpu`, in a child process) and on the device (`gpu`)."""
import numpy as np

from vins_mono_amd import fe, synth

import e2e_vio
from fe_read_image_batch_case import status_of
from fe_tracks_case import LONG_MIN_DIST, _long_streams, same_state, same_tracks_out, step_args
from seq_imu_model import noise_of, resampled, rows_of

REFUSALS = ["begin without IMU mode", "begin with n_cams != nwin", "begin with max_points > max_new_obs", "begin with unknown flags",
            "struct_size", "n != n_cams", "mixed publish", "no samples on a publishing frame", "more samples than max_samples",
            "samples on a frame that does not publish", "a sample that is not finite", "struct_size of the front end's part",
            "max_cnt > max_points", "mixed equalize", "callback failure", "step after vio_end", "step after tracks_begin", "step after seq_end"]


def release(*handles):
    """end bridge and sequence of every handle, whatever state a failed case left them in (the handles outlive the case; an error
    of the clean-up must not hide the case's own)"""
    for h in handles:
        for end in (h.vio_end, h.seq_end):
            try:
                end()
            except RuntimeError as e:
                print("clean-up:", e)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (what, a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# case 1: the staged frame equals the message
def _empty_windows(n, K, max_iters=2):
    """n synthetic windows without tracks (every track comes from the front end, as in `vins_replay vio`) and their sample sources"""
    srcs = [synth.FrameSource(synth.SyntheticSequence(40 + w, n_frames=K + 8, K=K + 8, L=10), noise_seed=900 + w) for w in range(n)]
    wins = [s.initial_window(K, 0) for s in srcs]
    for w in wins:
        w['tracks'] = []
        w['base'] = dict(w['base'], max_iters=max_iters)
    return srcs, wins


def _begin_estimator(h, srcs, wins, K, max_features, max_new_obs, max_samples, min_parallax=10.0 / 460.0):
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
    h.seq_begin(list(probs), list(trks), max_features=max_features, max_new_obs=max_new_obs, init_depth=5.0, min_parallax=min_parallax)
    seeds = []
    for s, w in zip(srcs, wins):
        last = w['samples'][K - 3][-1]                                    # the measurement at the newest frame of the window
        seeds.append(np.concatenate([last[1], last[2], [0.0, 0.0, s.seq.cfg['g_norm']]]))
    h.seq_imu_begin(seeds, noise_of(srcs[0].seq), max_samples=max_samples)


def _staged(h_a, h_b, name, sds, max_cnt, cap, min_dist, targets, seen):
    """streams `sds` on both handles, every frame publishing; h_a through vio_step with VG_VIO_LISTS, h_b through tracks_step.
    targets[c]: n_msg of stream c in the last frame.  The message holds the carried points, so h_b first runs that frame with the full
    lists to learn which points survive it, goes back one frame (push_frames + tracks_begin + tracks_set, as a caller that re-seeds),
    and both handles get lists cut down to the first targets[c] survivors.  A point's tracking does not depend on the other points, a
    subset of points that setMask kept is kept again, and with an F_THRESHOLD of 1e6 px rejectWithF removes nothing: the cut lists
    survive whole."""
    W, H, K, n_frames = 320, 240, 4, 4
    streams = _long_streams(sds, max_cnt, n_frames, W, H)
    S, last = len(streams), n_frames - 1
    tra, trb = fe.FrontEnd(h_a, W, H, S, cap), fe.FrontEnd(h_b, W, H, S, cap)
    tra.tracks_begin(); trb.tracks_begin()
    srcs, wins = _empty_windows(S, K)
    _begin_estimator(h_a, srcs, wins, K, 1024, cap, 20)
    h_a.vio_begin(lists=True)

    def args(k):
        a = step_args(streams, k, min_dist)
        a["publish_list"], a["f_threshold"] = [True] * S, [1e6] * S
        return a

    try:
        for k in range(n_frames):
            if k == last:
                st = [trb.tracks_get(c) for c in range(S)]
                dry = trb.tracks_step(**args(k))
                trb.push_frames([s.frames[k - 1] for s in streams], equalize=True)
                trb.tracks_begin()
                for c in range(S):
                    assert dry[c]["n_msg"] >= targets[c], (name, "too few survivors for the case", c, dry[c]["n_msg"], targets[c])
                    keep = np.isin(st[c]["ids"], dry[c]["msg_id"][:targets[c]])
                    for tr in (tra, trb):
                        tr.tracks_set(c, st[c]["cur_xy"][keep], st[c]["ids"][keep], st[c]["track_cnt"][keep], st[c]["n_id"], st[c]["prev_time"],
                                      st[c]["un_xy"][keep], st[c]["in_map"][keep])
            oa = h_a.vio_step(tra, [rows_of(srcs[w].samples(K - 2 + k)) for w in range(S)], **args(k))
            ob = trb.tracks_step(**args(k))
            n_msg = []
            for c in range(S):
                what = (name, "frame", k, "stream", c)
                same_tracks_out(oa[c], ob[c], what)
                ids, obs = h_a.vio_frame(c, cap)
                print("vio staged", what, "n_msg", oa[c]["n_msg"], "staged", len(ids))
                for other in (oa[c], ob[c]):
                    same_bits(ids, other["msg_id"], what + ("ids",))
                    same_bits(obs, other["msg_obs"], what + ("rows",))
                n_msg.append(oa[c]["n_msg"])
            seen["n_msg"].update(n_msg)
            if 0 in n_msg and max(n_msg) > 0:
                seen["empty_beside_messages"] += 1
            if S == 3 and len(set(n_msg)) == 3:
                seen["three_different"] += 1
    finally:
        release(h_a)


def run_staged(h_a, h_b):
    """three streams with an empty message, 260 and 100 rows in one call (max_points 400: ids in 16-byte copies, more than one pass of
    the 256 threads, more than four tiles of 64 rows), then 64 and 65 rows at max_points 161 (odd: scalar id copies, and the second
    stream's rows start at an odd double)"""
    seen = dict(n_msg=set(), empty_beside_messages=0, three_different=0)
    _staged(h_a, h_b, "long", (4, 5, 6), (400, 400, 400), 400, LONG_MIN_DIST, (0, 260, 100), seen)
    _staged(h_a, h_b, "edge", (4, 5), (100, 100), 161, 14, (64, 65), seen)
    return dict(n_msg=sorted(seen["n_msg"]), empty_beside_messages=seen["empty_beside_messages"], three_different=seen["three_different"])


def check_staged(seen):
    n = seen["n_msg"]
    assert 0 in n and 64 in n and 65 in n and max(n) > 256, seen
    assert seen["empty_beside_messages"] >= 1 and seen["three_different"] >= 1, seen


# ---------------------------------------------------------------------------------------------------------------------------
# cases 2, 3, 5: two rendered camera + IMU streams (tests/e2e_vio.py's Scene with two seeds) through front end and estimator
class Data:
    """The frames of two scenes and what seeds the estimators.  K frames per window; g0 frames of front-end warm-up in front of the
    window (K = 4 needs one: a landmark of a 4-frame window must start in its first frame, and nothing is published before a track is
    two frames old); half: frames at 376x240 (the emulator's size), 2x2 means of the rendered 752x480 ones."""

    def __init__(self, K, g0, half, seeds=(3, 4), plan="PPNPP"):
        self.K, self.g0, self.plan, self.S = K, g0, plan, len(seeds)
        n_frames = g0 + K - 1 + len(plan)
        self.scenes = [e2e_vio.Scene(s, n_frames) for s in seeds]
        c = self.scenes[0].seq.cfg
        sc = 0.5 if half else 1.0
        self.W, self.H, self.min_dist = int(752 * sc), int(480 * sc), int(30 * sc)
        self.intr = (c['fx'] * sc, c['fy'] * sc, c['cx'] * sc, c['cy'] * sc) + tuple(e2e_vio.K_DIST[k] for k in ('k1', 'k2', 'p1', 'p2'))
        self.frames = []
        for s in self.scenes:
            fr = [s.render(f) for f in range(n_frames)]
            if half:
                fr = [np.rint(f.reshape(240, 2, 376, 2).astype(np.float64).mean(axis=(1, 3))).astype(np.uint8) for f in fr]
            self.frames.append(fr)
        self.srcs = [synth.FrameSource(s.seq, noise_seed=5) for s in self.scenes]

    def fe_args(self, f, publish):
        return dict(imgs=[fr[f] for fr in self.frames], stamps=[0.05 * f] * self.S, publish_list=[publish] * self.S, intr_list=[self.intr] * self.S,
                    max_cnt=150, min_dist=self.min_dist, equalize=True, f_threshold=1.0, focal_length=460.0)

    def windows(self, msgs):
        """the seeded windows, as tests/e2e_vio.py run_estimator builds them, from the messages of frames g0 .. g0 + K - 2"""
        K, g0, wins = self.K, self.g0, []
        for c, scene in enumerate(self.scenes):
            seq, src = scene.seq, synth.FrameSource(scene.seq, noise_seed=5)
            pose, sb = zip(*[src.guess(g0 + i) for i in range(K - 1)])
            pose, sb = list(pose) + [pose[-1]], list(sb) + [sb[-1]]
            smp = [src.samples(g0 + i) for i in range(K - 2)] + [None]
            imu = [src.preintegrate(s, seq.ba_lin, seq.bg_lin) for s in smp[:-1]] + [None]
            feats = {}
            for f in range(K - 1):
                ids, obs = msgs[g0 + f][c]
                for fid, r in zip(ids, obs):
                    ft = feats.setdefault(int(fid), dict(id=int(fid), start=f, obs=[], depth=-1.0))
                    ft['obs'].append(list(r) + [0.0])
            wins.append(dict(K=K, base=seq._base(), pose=np.array(pose), sb=np.array(sb), imu=imu, samples=smp, tracks=list(feats.values())))
        return wins


class Rig:
    """one handle: a front end of two streams with resident lists and a sequence of two windows in IMU mode, seeded after the warm-up"""

    def __init__(self, h, data, max_new_obs=512, imu=True, max_samples=32, per_frame=None):
        """per_frame: IMU rows per frame interval (None: the 10 of the scene's sample source; else the interval re-sampled)"""
        self.h, self.d, self.per_frame = h, data, per_frame
        self.tr = fe.FrontEnd(h, data.W, data.H, data.S, 150)
        self.tr.tracks_begin()
        self.msgs = []
        for f in range(data.g0 + data.K - 1):
            outs = self.tr.tracks_step(**data.fe_args(f, True))
            self.msgs.append([(o["msg_id"], o["msg_obs"]) for o in outs])
        self.wins = data.windows(self.msgs)
        if imu:
            _begin_estimator(h, data.srcs, self.wins, data.K, 768, max_new_obs, max_samples)
        self.pending = [np.zeros((0, 7))] * data.S
        self.f = data.g0 + data.K - 1

    def _samples(self):
        """the rows since the previous PUBLISHED frame, as getMeasurements pairs them"""
        f, n = self.f, self.per_frame
        self.pending = [np.concatenate([p, rows_of(s.samples(f - 1)) if n is None else resampled(s, f - 1, n)]) for p, s in zip(self.pending, self.d.srcs)]

    def old_step(self, publish):
        self._samples()
        outs = self.tr.tracks_step(**self.d.fe_args(self.f, publish))
        if publish:
            self.h.seq_step_imu([dict(samples=p, ids=o["msg_id"], obs=o["msg_obs"]) for p, o in zip(self.pending, outs)])
            self.pending = [np.zeros((0, 7))] * self.d.S
        self.f += 1
        return outs

    def vio_step(self, publish, **over):
        self._samples()
        a = dict(self.d.fe_args(self.f, publish), **over)
        outs = self.h.vio_step(self.tr, self.pending if publish else None, **a)
        if publish:
            self.pending = [np.zeros((0, 7))] * self.d.S
        self.f += 1
        return outs

    def snapshot(self):
        K, S = self.d.K, self.d.S
        states, sums = self.h.seq_states()
        return dict(states=states, sums=sums, info=self.h.seq_info(), tracks=[self.h.seq_tracks(w, K) for w in range(S)],
                    imu=[self.h.seq_imu_get(w) for w in range(S)])

    def lists(self):
        return [self.tr.tracks_get(c) for c in range(self.d.S)]


def same_snapshot(a, b, what):
    """states, summaries, all VG_SEQ_* info ints, vg_ba_seq_get_tracks and vg_ba_seq_imu_get of every window"""
    assert a["info"] == b["info"], (what, a["info"], b["info"])
    for w in range(len(a["states"])):
        for k, v in a["states"][w].items():
            same_bits(np.asarray(v, np.float64), np.asarray(b["states"][w][k], np.float64), what + (w, "state", k))
        for k, v in a["sums"][w].items():
            if k == "prof":                                              # (device phase timers of a profiling build: shader cycles)
                continue
            same_bits(np.asarray(v), np.asarray(b["sums"][w][k]), what + (w, "summary", k))
        for k, v in a["tracks"][w].items():
            same_bits(v, b["tracks"][w][k], what + (w, "tracks", k))
        for k, v in a["imu"][w].items():
            same_bits(v, b["imu"][w][k], what + (w, "imu", k))


def run_pair(h_a, h_b, data, lists, how):
    """handle A on the one-call path, handle B on the two old calls, from the same seeded state.  how = "bridged": every frame of A
    through vio_step; "interleaved": vio_step, the two old calls, vio_step, ... on A.  Compared after every publishing frame."""
    try:
        a, b = Rig(h_a, data), Rig(h_b, data)
        for f in range(len(a.msgs)):
            for c in range(data.S):
                same_bits(a.msgs[f][c][0], b.msgs[f][c][0], ("warm-up ids", f, c))
                same_bits(a.msgs[f][c][1], b.msgs[f][c][1], ("warm-up rows", f, c))
        h_a.vio_begin(lists=lists)
        flags, nulls, n_pub = [], 0, 0
        for k, p in enumerate(data.plan):
            publish = p == "P"
            bridged = how == "bridged" or k % 2 == 0
            oa = a.vio_step(publish) if bridged else a.old_step(publish)
            ob = b.old_step(publish)
            what = (how, "lists" if lists else "counts", "step", k)
            for c in range(data.S):
                if bridged and not lists:
                    assert sorted(oa[c]["null_pointers"]) == sorted(["ids", "track_cnt", "cur_xy", "un_xy", "vel_xy", "msg_id", "msg_obs"]), (what, oa[c])
                    nulls += 1
                    for key in ("n", "n_id", "n_msg", "n1", "n2", "ransac_ran", "n_kept", "n_new", "fallback", "ransac_best", "ransac_niters"):
                        assert oa[c][key] == ob[c][key], (what, c, key, oa[c][key], ob[c][key])
                else:
                    same_tracks_out(oa[c], ob[c], what + (c,))
            for la, lb in zip(a.lists(), b.lists()):
                same_state(la, lb, what + ("lists",))
            if not publish:
                continue
            n_pub += 1
            sa, sb = a.snapshot(), b.snapshot()
            same_snapshot(sa, sb, what)
            if bridged:
                for c in range(data.S):
                    ids, obs = h_a.vio_frame(c, 150)
                    same_bits(ids, ob[c]["msg_id"], what + (c, "staged ids"))
                    same_bits(obs, ob[c]["msg_obs"], what + (c, "staged rows"))
            for w in range(data.S):
                assert sa["info"][w]["status"] == 0 and sa["sums"][w]["status"] == 0, (what, w, sa["info"][w], sa["sums"][w]["status"])
            flags.append([i["flag"] for i in sa["info"]])
            print("vio pair", what, "flags", flags[-1], "n_msg", [o["n_msg"] for o in ob], "landmarks", [i["n_landmarks"] for i in sa["info"]])
        return dict(flags=flags, publishing=n_pub, null_outputs=nulls, non_publishing=data.plan.count("N"))
    finally:
        release(h_a, h_b)


def run_regrow(h_a, h_b, data):
    """a bridge begun at max_samples 16, vg_ba_seq_imu_begin again at 64 on the running sequence (it ends the bridge and replaces the
    staging), the bridge begun again, then a published frame behind two unpublished ones: 33 rows, more than the first capacity.  11
    rows per frame interval, so that every count is odd (the sample copy of the bridge kernel ends in a half pair)."""
    try:
        a, b = Rig(h_a, data, max_samples=16, per_frame=11), Rig(h_b, data, max_samples=16, per_frame=11)
        noise = noise_of(data.srcs[0].seq)
        counts = []

        def step(publish, what):
            n = [len(p) + 11 for p in a.pending]
            oa, ob = a.vio_step(publish), b.old_step(publish)
            for c in range(data.S):
                same_tracks_out(oa[c], ob[c], what + (c,))
            if publish:
                sa, sb = a.snapshot(), b.snapshot()
                same_snapshot(sa, sb, what)
                for c in range(data.S):
                    ids, obs = h_a.vio_frame(c, 150)
                    same_bits(ids, ob[c]["msg_id"], what + (c, "staged ids"))
                    same_bits(obs, ob[c]["msg_obs"], what + (c, "staged rows"))
                    assert sa["info"][c]["status"] == 0 and sa["sums"][c]["status"] == 0, (what, c, sa["info"][c], sa["sums"][c]["status"])
                counts.append(n[0])

        h_a.vio_begin(lists=True)
        step(True, ("regrow", "at 16"))
        for r in (a, b):
            seeds = [np.concatenate([m["acc_0"], m["gyr_0"], m["g"]]) for m in (r.h.seq_imu_get(w) for w in range(data.S))]
            r.h.seq_imu_begin(seeds, noise, max_samples=64)
        f, pend = a.f, a.pending
        a._samples()
        try:
            h_a.vio_step(a.tr, a.pending, **data.fe_args(f, True))
            raise AssertionError("the bridge survived vg_ba_seq_imu_begin")
        except RuntimeError as e:
            assert status_of(e) == -1, str(e)
        a.f, a.pending = f, pend
        h_a.vio_begin(lists=True)
        step(False, ("regrow", "unpublished 1"))
        step(False, ("regrow", "unpublished 2"))
        step(True, ("regrow", "at 64"))
        step(True, ("regrow", "after"))
        return dict(samples=counts)
    finally:
        release(h_a, h_b)


def check_pair(seen, lists):
    flat = [f for row in seen["flags"] for f in row]
    assert seen["publishing"] >= 4 and seen["non_publishing"] >= 1 and 0 in flat and 1 in flat, seen      # both marginalization flags occurred
    assert lists or seen["null_outputs"] > 0, seen


# ---------------------------------------------------------------------------------------------------------------------------
# case 4: refusals
def run_refusals(h, data):
    done = []

    def refused(name, fn, code=-1):
        try:
            fn()
        except RuntimeError as e:
            assert status_of(e) == code and len(str(e)) > 40, (name, str(e))
            done.append(name)
            return
        raise AssertionError("not refused: " + name)

    # ---- vg_vio_begin
    r = Rig(h, data, imu=False)
    probs, trks = zip(*[synth.sequence_inputs(w) for w in r.wins])
    h.seq_begin(list(probs), list(trks), max_features=768, max_new_obs=512, init_depth=5.0)
    refused("begin without IMU mode", lambda: h.vio_begin())
    h.seq_end()
    _begin_estimator(h, data.srcs[:1], r.wins[:1], data.K, 768, 512, 32)
    refused("begin with n_cams != nwin", lambda: h.vio_begin())
    h.seq_end()
    _begin_estimator(h, data.srcs, r.wins, data.K, 768, 128, 32)
    refused("begin with max_points > max_new_obs", lambda: h.vio_begin())
    h.seq_end()
    _begin_estimator(h, data.srcs, r.wins, data.K, 768, 512, 32)
    refused("begin with unknown flags", lambda: h._chk(h.lib.vg_vio_begin(h.h, 2), "vg_vio_begin"))
    h.vio_begin()
    try:
        r.vio_step(True)                                                    # one good step: lists and windows hold a frame's work
        lists0, snap0 = r.lists(), r.snapshot()

        def nothing_moved(name):
            for c, (la, lb) in enumerate(zip(r.lists(), lists0)):
                same_state(la, lb, (name, "lists", c))
            same_snapshot(r.snapshot(), snap0, (name,))

        def bad_step(name, publish=True, samples=None, **over):
            f, pend = r.f, r.pending
            r._samples()
            smp = r.pending if samples is None else samples
            r.f, r.pending = f, pend
            a = dict(data.fe_args(f, publish), **over)
            refused(name, lambda: h.vio_step(r.tr, smp if (publish or samples is not None) else None, **a))
            nothing_moved(name)

        S = data.S
        ten = rows_of(data.srcs[0].samples(r.f - 1))
        bad_step("struct_size", vio_struct_size=8)
        bad_step("n != n_cams", n_streams=S + 1)
        bad_step("mixed publish", publish_list=[True] + [False] * (S - 1))
        bad_step("no samples on a publishing frame", samples=[ten] + [None] * (S - 1))
        bad_step("more samples than max_samples", samples=[ten] * (S - 1) + [np.concatenate([ten] * 4)])
        bad_step("samples on a frame that does not publish", publish=False, samples=[ten] * S)
        nan = ten.copy(); nan[-1, 6] = np.nan
        bad_step("a sample that is not finite", samples=[ten] * (S - 1) + [nan])
        bad_step("struct_size of the front end's part", struct_size=8)
        bad_step("max_cnt > max_points", max_cnt=[150] * (S - 1) + [151])
        bad_step("mixed equalize", equalize=[True] + [False] * (S - 1))
        r.vio_step(True)                                                    # the bridge is as usable as before
        # ---- the front end fails after its upload: the estimator part is not launched, lists and windows stay (the frames are one ahead)
        lists0, snap0 = r.lists(), r.snapshot()

        def failing(cnt):
            raise RuntimeError("the caller's sort failed")

        bad_step("callback failure", orders=[None] * (S - 1) + [failing])
        # ---- what ends the bridge
        h.vio_end()
        lists0, snap0 = r.lists(), r.snapshot()
        bad_step("step after vio_end")
        h.vio_begin()
        r.tr.tracks_begin()
        f, pend = r.f, r.pending
        r._samples()
        refused("step after tracks_begin", lambda: h.vio_step(r.tr, r.pending, **data.fe_args(f, True)))
        same_snapshot(r.snapshot(), snap0, ("step after tracks_begin",))
        h.vio_begin()
        h.seq_end()
        refused("step after seq_end", lambda: h.vio_step(r.tr, r.pending, **data.fe_args(f, True)))
    finally:
        release(h)
    return done
