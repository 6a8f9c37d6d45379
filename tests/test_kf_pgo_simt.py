"""vg_pg_optimize through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/kf_pgo.h compiled for the CPU fiber emulator), and
the checks of the restatement itself.  Reference, cases, metric and the check bodies are tests/kf_pgo_ref.py; tests/test_kf_pgo_gpu.py runs
the same bodies on the MI355X."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import conftest
import kf_pgo_ref as K

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return K.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(K.CASE_ARGS)


def test_cases_reach_what_they_are_there_for():
    K.check_case_properties()


def test_batch_equals_single_graphs(simt_handle):
    K.check_batch_equals_single(simt_handle, (1, 3, 33))


def test_failed_graph_leaves_its_neighbours(simt_handle):
    K.check_failed_neighbours(simt_handle)


@pytest.mark.parametrize("name", K.REFUSALS)
def test_refusal(simt_handle, name):
    K.check_refusal(simt_handle, name)


def test_chain_from_the_pnp_stage(simt_handle):
    K.check_chain(simt_handle)


@pytest.mark.parametrize("name", K.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """PoseGraph::addKeyFrame's pose bookkeeping and optimize4DoF (host/pose_graph.h, vg_pack_pg) through `vins_replay_simt pgo`"""
    conftest._build_simt()
    K.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


# ---- the restatement itself, on the CPU
def test_mutations_are_told_apart():
    """each mutated restatement (Huber's scaling dropped, the yaw row's 1/10 dropped, pi/180 dropped, the Jacobi scale recomputed every
    iteration, the CG tolerance at 1e-3, the tail's drift left out, sequence 0 free, the candidate's residuals kept behind a rejected
    step) is told from the definition by at least one case; normalising a chain edge's relative_yaw is equivalent and told by none"""
    caught = K.check_mutations()
    assert 'rejected' in caught['rescale_every_iteration'] and 'rejected' in caught['candidate_residuals_kept']


def test_jacobian_against_central_differences():
    """Ja, Jb of every edge slot of n40_four (chain and Huber-scaled loop edges) against central differences of the corrected residual with
    the corrector's scale held (Ceres differentiates the functor; the corrector multiplies afterwards)"""
    g = dict(K.case('n40_four'))
    G0 = K.Graph(g, np.float64, edit='no_huber')
    rng = np.random.default_rng(5)
    yaw, t = G0.yaw0 + rng.normal(0, 0.5, G0.N), G0.t0 + rng.normal(0, 0.05, (G0.N, 3))
    s_loop = np.sort((G0.evaluate(yaw, t, False)[1][G0.valid & G0.loop] ** 2).sum(1))
    g['huber_delta'] = float(np.sqrt(0.5 * (s_loop[1] + s_loop[2])))      # two of the four loop edges on each branch of Huber
    G = K.Graph(g, np.float64)
    _, res, Ja, Jb, hub = G.evaluate(yaw, t, True)
    assert hub.sum() == 2 and (~hub & G.valid & G.loop).sum() == 2
    G2 = K.Graph(g, np.float64, edit='no_huber')            # the raw functor
    _, _, Ja0, Jb0, _ = G2.evaluate(yaw, t, True)
    h = 1e-6
    for role, J0 in (('a', Ja0), ('b', Jb0)):
        for k in range(4):
            num = np.zeros((5 * G.N, 4))
            for e in np.nonzero(G.valid)[0]:
                node = G.a[e] if role == 'a' else G.b[e]
                yp, ym, tp, tm = yaw.copy(), yaw.copy(), t.copy(), t.copy()
                if k == 0:
                    yp[node] += h; ym[node] -= h
                else:
                    tp[node, k - 1] += h; tm[node, k - 1] -= h
                rp, rm = G2.evaluate(yp, tp, False)[1][e], G2.evaluate(ym, tm, False)[1][e]
                num[e] = (rp - rm) / (2 * h)
            assert np.abs(num - J0[:, :, k]).max() < 1e-7, (role, k)
    # the corrector: rows times sqrt(rho'), nothing else
    s = np.where(hub, np.sqrt(G.delta / np.sqrt(np.maximum((G2.evaluate(yaw, t, False)[1] ** 2).sum(1), 1e-300))), 1.0)
    assert np.allclose(Ja, Ja0 * s[:, None, None], rtol=1e-14, atol=0) and np.allclose(Jb, Jb0 * s[:, None, None], rtol=1e-14, atol=0)


def test_pcg_step_equals_the_dense_step():
    """every trace row of every case: the preconditioned-CG step against numpy.linalg.solve on the same system, relative 1e-10"""
    for name in K.CASE_ARGS:
        steps = []
        K.solve(K.case(name), 'pcg64', steps=steps)
        for A, b, y in steps:
            yd = np.linalg.solve(A, b)
            assert np.linalg.norm(y - yd) <= 1e-10 * np.linalg.norm(yd), name


def test_final_cost_against_scipy():
    """the dense64 route's result against scipy.optimize.least_squares(loss='huber', f_scale=huber_delta) run to convergence from it.
    scipy applies its loss to every residual row on its own, so a loop edge enters as ONE row, the norm of its four residuals (then
    f_scale^2 rho((f / f_scale)^2) is Ceres' Huber of s), and a chain edge as its four rows, which must stay below huber_delta, where
    scipy's Huber is the identity (asserted at both ends).  The cost may not rise, and where the run ended by tolerance it may not fall
    by more than the function tolerance allows after 5 iterations."""
    from scipy.optimize import least_squares
    for name in ('n12_one', 'tail', 'in_band_loop', 'wrap', 'n40_four', 'seq0_constant'):
        g = K.case(name)
        ref = K.reference(name, 'dense64')
        G = K.Graph(g, np.float64, edit='no_huber')             # the raw functor rows
        delta = float(G.delta)
        yaw0, t0 = K.R2ypr(ref['R'][:G.N], np.float64)[:, 0], np.asarray(ref['T'][:G.N], np.float64)
        x0 = np.concatenate([yaw0[G.nof], t0[G.nof].reshape(-1)])
        chain, loop = G.valid & ~G.loop, G.valid & G.loop

        def rows(x):
            yaw, t = yaw0.copy(), t0.copy()
            yaw[G.nof], t[G.nof] = x[:G.NF], x[G.NF:].reshape(-1, 3)
            e = G.evaluate(yaw, t, False)[1]
            return np.concatenate([e[chain].reshape(-1), np.sqrt((e[loop] ** 2).sum(1))])
        n_chain = 4 * int(chain.sum())
        assert np.abs(rows(x0)[:n_chain]).max() < delta, name
        c0 = least_squares(rows, x0, loss='huber', f_scale=delta, max_nfev=1).cost
        assert abs(c0 - ref['final_cost']) <= 1e-12 * ref['initial_cost'], (name, c0, ref['final_cost'])
        sol = least_squares(rows, x0, loss='huber', f_scale=delta, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
        assert np.abs(rows(sol.x)[:n_chain]).max() < delta, name
        print(f"kf_pgo scipy {name}: final cost {c0:.12g}, least_squares {sol.cost:.12g}, relative fall {(c0 - sol.cost) / c0:.3g}")
        assert sol.cost <= c0 * (1 + 1e-12), name
        if ref['termination'] == K.CONVERGENCE:
            # the run ended because a step changed the cost by at most 1e-6 of it: with the steps shrinking geometrically (the ratio of
            # the last two cost changes of the trace, at most 1/10 on these cases) what is left is a small multiple of that
            assert c0 - sol.cost <= 1e-5 * c0, (name, c0, sol.cost)


def test_standalone_sanitizer_run(simt_handle, tmp_path):
    """tests/kf_pgo_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on four
    cases: no report, the batch equals the single calls, and the decisions equal the unsanitized run through the binding"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "kf_pgo_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "kf_pgo_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    names, files = ('n12_one', 'n60_two_seq', 'tail', 'no_free'), []
    for name in names:
        files.append(str(tmp_path / (name + ".bin")))
        K.write_file(files[-1], K.case(name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * len(names)
    got = K._fe().pg_optimize(simt_handle, [K.case(n) for n in names])
    for a, b, g in zip(rows[:len(names)], rows[len(names):], got):
        assert a[0] == 'batch' and b[0] == 'alone' and a[1:] == b[1:]
        assert [int(x) for x in a[1:7]] == [g[k] for k in K.DECISIONS]
        assert float.fromhex(a[7]) == g['final_cost'] and float.fromhex(a[8]) == g['yaw_drift']
