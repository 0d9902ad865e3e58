"""Hierarchical sampler on the GPU (-m gpu): log_target_distribution against the reference golden vectors, chains
bit-identical to the CPU twin, the --hierarchical command line and its files."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, rows_of

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def dr_setup():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return dr


def test_prior_parameters_match_reference():
    from pyhillfit_amd import hierarchical as H
    g = np.load(os.path.join(GOLDEN, "g2_hier_target.npz"))
    shapes, scales, locs = H.prior_params()
    assert np.array_equal(shapes, g["shapes"]) and np.array_equal(scales, g["scales"]) and np.array_equal(locs, g["locs"])


def test_hier_log_target_vs_reference_golden_and_twin(gpu, golden_meta, oracle_pair):
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    g = np.load(os.path.join(GOLDEN, "g2_hier_target.npz"))
    shapes, scales, locs = H.prior_params()
    done = 0
    for ip, m in enumerate(golden_meta["g2_pairs"]):
        if m["Ne"] > H.MAX_EXPTS:
            continue
        p = oracle_pair(m["drug"], m["channel"], m["file"])
        packed = H.PackedHierPoints([p.experiments])
        th = g["theta_%d" % ip]
        got = H.log_target_batch(packed, np.zeros(len(th), dtype=np.int32), th, device=gpu)
        want = g["target_%d" % ip]
        bad = ~np.isfinite(want)
        assert np.array_equal(got[bad], want[bad], equal_nan=True)
        np.testing.assert_allclose(got[~bad], want[~bad], rtol=1e-12, atol=0)
        pk = co.PackedHierPair(p.experiments, shapes, scales, locs)
        assert np.array_equal(got, np.array([pk.log_target(t) for t in th]), equal_nan=True)
        done += 1
    assert done == 8          # includes the synthetic Ne = 50 pair (dim 105) through the generic-Ne kernel


@pytest.mark.parametrize("names", [[("Amiodarone", "hERG"), ("Lidocaine", "KvLQT1/mink")], [("Amitriptyline", "Kv4.3"), ("Cibenzoline", "Kv4.3")]])
def test_hier_chains_bit_identical_to_cpu_twin(names, gpu, oracle_pair):
    """Ne = 3 (dim 11) and Ne = 6 (dim 17): same seed => same chain and final state bit for bit, launches cut unevenly"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    pairs = [oracle_pair(d, c) for d, c in names]
    packed = H.PackedHierPoints([p.experiments for p in pairs])
    ne = packed.n_expts
    d = 5 + 2 * ne
    theta0 = np.array([np.concatenate([[1., 5., 6., .3], np.tile([6.0, 0.8], ne), [8.0]]),
                       np.concatenate([[1.2, 4., 5., .4], np.tile([4.5, 1.1], ne), [5.0]])])
    C, T, thin, adapt = 70, 700, 5, 150
    s = H.HierarchicalSampler(packed, [0, 1], C, thinning=thin, seed=987654321, adapt_start=adapt, problem_ids=[11, 12],
                              chain_id_base=5, device=gpu)
    s.init(theta0, cov_scale=0.01)
    row0 = s.row0.cpu().numpy()
    parts = [s.advance(k).cpu().numpy() for k in (adapt - 3, 4, T - adapt - 1)]
    chain = np.concatenate(parts)
    assert chain.shape == (T // thin, 2, d + 1, C)
    state = s.state.cpu().numpy().reshape(s.S, 2, C)
    gam = gamma_table(T)
    for q in range(2):
        pk = co.PackedHierPair(pairs[q].experiments, shapes, scales, locs)
        for c in (0, 33, C - 1):
            st = pk.init_state(theta0[q], 0.01)
            assert np.array_equal(row0[q, :, c], np.concatenate([theta0[q], [st[d]]]))
            rows = pk.advance(st, 0, T, thin, adapt, gam, seed=987654321, chain_id=5 + c, problem_id=11 + q)
            assert np.array_equal(chain[:, q, :, c], rows), (q, c)
            assert np.array_equal(state[:, q, c], st), (q, c)
    assert 0.01 < float(s.acceptance().mean()) < 0.95


@pytest.mark.parametrize("names", [[("Amiodarone", "hERG"), ("Verapamil", "hERG")],            # Ne = 3: 4+4+4 points (straight-line body) and 5+5+4
                                   [("Amiodarone", "Nav1.5-peak"), ("Amiodarone", "Kv4.3")],   # Ne = 4: 4+4+4+1 and 4+4+4+3
                                   [("Moxifloxacin", "KvLQT1/mink"), ("Dofetilide", "hERG")],  # Ne = 5: 4 points each (straight-line) and 5+5+4+2+2
                                   [("Amitriptyline", "Kv4.3"), ("Cibenzoline", "Kv4.3")]])    # Ne = 6: 4+4+4+4+2+1 and 4+4+4+1+1+1
def test_two_lanes_per_chain_kernel_is_bit_identical(names, gpu, oracle_pair):
    """hier_advance2_kernel<Ne, WPS> (two lanes share a chain: rows of the state, Philox blocks and the halves of the target split
    between them, 32 chains per wavefront; WPS 1: 512 registers, every table resident — the build small launches run; WPS 2: 256
    registers, tables and prior through LDS, two wavefronts per SIMD) against hier_advance_kernel<Ne> (one lane per chain) and
    the twin: same chain, same final state, same moments, bit for bit; H.set_kernel_policy forces kernel and build"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    pairs = [oracle_pair(d, c) for d, c in names]
    packed = H.PackedHierPoints([p.experiments for p in pairs])
    ne = packed.n_expts
    d = 5 + 2 * ne
    theta0 = np.array([np.concatenate([[1., 5., 6., .3], np.tile([6.0, 0.8], ne), [8.0]]),
                       np.concatenate([[1.2, 4., 5., .4], np.tile([4.5, 1.1], ne), [5.0]])])
    C, T, thin, adapt = 200, 600, 5, 140              # 200 chains: a ragged last wavefront for both kernels (64 and 32 chains each)
    got = {}
    for wps in ("1", "2", "2/2"):
        H.set_kernel_policy(lanes=int(wps[0]), wps=2 if wps == "2/2" else 1)
        s = H.HierarchicalSampler(packed, [0, 1], C, thinning=thin, seed=31337, adapt_start=adapt, problem_ids=[4, 5], chain_id_base=64, device=gpu)
        s.init(theta0, cov_scale=0.01)
        s.enable_moments(after_iteration=adapt)
        chain = np.concatenate([s.advance(k).cpu().numpy() for k in (adapt + 7, T - adapt - 7)])
        mean, var, n = s.posterior_moments()
        got[wps] = (chain, s.state.cpu().numpy().reshape(s.S, 2, C), mean.cpu().numpy())
    H.set_kernel_policy(0, 0)
    for other in ("2", "2/2"):
        assert all(np.array_equal(got["1"][i], got[other][i]) for i in range(3)), other
    chain, state, mean = got["2"]
    keep = chain[(adapt // thin):]                                            # rows saved at t > adapt
    np.testing.assert_allclose(mean, keep.mean(axis=0).transpose(1, 0, 2), rtol=1e-12, atol=1e-12)
    gam = gamma_table(T)
    for q in range(2):
        pk = co.PackedHierPair(pairs[q].experiments, shapes, scales, locs)
        for c in (0, 31, 32, 63, 64, C - 1):
            st = pk.init_state(theta0[q], 0.01)
            rows = pk.advance(st, 0, T, thin, adapt, gam, seed=31337, chain_id=64 + c, problem_id=4 + q)
            assert np.array_equal(chain[:, q, :, c], rows), (q, c)
            assert np.array_equal(state[:, q, c], st), (q, c)


@pytest.mark.parametrize("lanes", [1, 2])
def test_zero_variance_direction_behaves_like_the_twin(lanes, gpu, oracle_pair):
    """a start point with a component exactly 0: the initial covariance 0.01 diag|theta0| (PyHillFit.py:431) has a zero row and
    column — d_k = 0 in the L diag(d) L' factors — so that component is never proposed away from its start and the reference's
    recursion (:498-499) keeps the row at zero: the component is frozen, in the reference as here.  What must hold: no division
    by zero (dn = 0 leaves column and alpha alone), everything else adapts, kernels == twin bit for bit incl. the final factors"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    p = oracle_pair("Amiodarone", "hERG")
    packed = H.PackedHierPoints([p.experiments])
    d = 11
    theta0 = np.array([1., 5., 6., .3, 6., .8, 6.1, .7, 0.0, .9, 8.])
    C, T, thin, adapt = 70, 500, 5, 50
    H.set_kernel_policy(lanes=lanes, wps=1)
    try:
        s = H.HierarchicalSampler(packed, [0], C, thinning=thin, seed=11, adapt_start=adapt, problem_ids=[3], device=gpu)
        s.init(theta0[None], cov_scale=0.01)
        chain = torch.cat([s.advance(adapt + 1), s.advance(T - adapt - 1)]).cpu().numpy()
        state = s.state.cpu().numpy().reshape(s.S, 1, C)
    finally:
        H.set_kernel_policy(0, 0)
    pk = co.PackedHierPair(p.experiments, shapes, scales, locs)
    for c in (0, 35, C - 1):
        st = pk.init_state(theta0, 0.01)
        rows = pk.advance(st, 0, T, thin, adapt, gamma_table(T), seed=11, chain_id=c, problem_id=3)
        assert np.array_equal(chain[:, 0, :, c], rows) and np.array_equal(state[:, 0, c], st), c

        assert np.all(rows[:, 8] == 0.0) and np.isfinite(st).all()
        cov = co.hier_state_covariance(st, d)
        assert np.all(cov[8] == 0.0) and np.all(np.delete(np.diag(cov), 8) > 0.0)


def test_policy_for_groups_running_side_by_side(gpu, oracle_pair):
    """hint_side_by_side: one lane per chain once the concurrent groups give every SIMD a wavefront, the library's own choice below
    that; the hint travels with the SAMPLER (phf_problems.kernel_hint) — another sampler of the same process is not affected —, a
    process-wide policy keeps the last word — and whichever kernel runs, the chain is the same bit for bit"""
    from pyhillfit_amd import hierarchical as H
    shapes, scales, locs = H.prior_params()
    p = oracle_pair("Amiodarone", "hERG")
    packed = H.PackedHierPoints([p.experiments])
    theta0 = np.array([H.first_iteration(p.experiments, locs)])
    assert H.simd_count() >= 64

    class Many(object):                                             # stands for the other groups of a full chip
        Q, C = H.simd_count(), 64

        def set_kernel_hint(self, lanes=0, wps=0):
            self.lanes = lanes

    def make():
        s = H.HierarchicalSampler(packed, [0], 64, thinning=5, seed=3, adapt_start=30, device=gpu)
        s.init(theta0, cov_scale=0.01)
        return s
    H.set_kernel_policy(0, 0)
    try:
        a, many = make(), Many()
        assert H.hint_side_by_side([a, many]) == 1 and (a.prob.kernel_hint & 63) == 1 and many.lanes == 1     # the chip is full: one lane (bit 6: the workspace's size, ABI 7)
        full = a.advance(100).cpu().numpy()
        b = make()
        assert (b.prob.kernel_hint & 63) == 0                       # a later sampler decides for itself: nothing process-wide was set
        assert H.hint_side_by_side([b]) == 0                        # one wavefront: the library's choice (two lanes)
        small = b.advance(100).cpu().numpy()
        c = make()
        c.set_kernel_hint(lanes=1)
        H.set_kernel_policy(2, 0)                                   # the process-wide policy overrides the hint
        forced = c.advance(100).cpu().numpy()
        with pytest.raises(ValueError):
            c.set_kernel_hint(lanes=3)
    finally:
        H.set_kernel_policy(0, 0)
    assert np.array_equal(full, small) and np.array_equal(forced, small)


@pytest.mark.parametrize("C", [1, 33])
def test_two_lane_kernel_with_one_chain_and_with_a_ragged_wavefront(C, gpu, oracle_pair):
    """what small command-line runs launch (the default policy picks the two-lane kernel): 1 chain (--num-chains 1: one lane pair of
    a wavefront) and 33 chains (a second wavefront with one pair active) against the twin, rows and moments"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    p = oracle_pair("Amiodarone", "hERG")
    packed = H.PackedHierPoints([p.experiments])
    d = 11
    theta0 = np.concatenate([[1., 5., 6., .3], np.tile([6.0, 0.8], 3), [8.0]])[None]
    T, thin, adapt = 400, 5, 120
    s = H.HierarchicalSampler(packed, [0], C, thinning=thin, seed=77, adapt_start=adapt, problem_ids=[9], device=gpu)
    s.init(theta0, cov_scale=0.01)
    s.enable_moments(after_iteration=adapt)
    chain = np.concatenate([s.advance(k).cpu().numpy() for k in (adapt + 3, T - adapt - 3)])
    mean, var, n = s.posterior_moments()
    pk = co.PackedHierPair(p.experiments, shapes, scales, locs)
    for c in sorted({0, C - 1}):
        st = pk.init_state(theta0[0], 0.01)
        rows = pk.advance(st, 0, T, thin, adapt, gamma_table(T), seed=77, chain_id=c, problem_id=9)
        assert np.array_equal(chain[:, 0, :, c], rows), c
        np.testing.assert_allclose(mean.cpu().numpy()[:, 0, c], rows[(adapt // thin):].mean(axis=0), rtol=1e-12, atol=1e-12)


def test_hierarchical_cli_and_statistics(gpu, tmp_path):
    """python PyHillFit.py --hierarchical: files where the reference puts them, (alpha, mu) consistent with the
    reference's stored samples (chaste/samples, coarse: 500 draws of an unseeded run)"""
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    out = str(tmp_path / "output")
    T = 60000
    summ = PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-i", str(T), "-t", "5", "--drugs", "Amiodarone,Dofetilide",
                           "--channels", "hERG", "--num-chains", "64", "--output-root", out, "--num-APs", "100"])
    assert len(summ) == 2
    with open(os.path.join(GOLDEN, "chaste_alpha_mu_stats.json")) as f:
        ref = json.load(f)
    for sm in summ:
        ne = sm["num_expts"]
        f = os.path.join(out, "crumb_data", "hierarchical", sm["drug"], "hERG", "%d_expts" % ne, "chain",
                         "crumb_data_%s_hERG_hierarchical_chain.txt" % sm["drug"])
        with open(f) as fh:
            assert fh.readline().startswith("# Hill ~ log-logistic(alpha,beta)") and fh.readline().startswith("# alpha, beta, mu, s")
        chain = np.loadtxt(f)
        assert chain.shape == (T // 5 + 1, 5 + 2 * ne + 1) and np.isfinite(chain[1:]).all()      # full chain, burn-in included (:514-515)
        samples = np.loadtxt(os.path.join(out, "crumb_data", "hierarchical", "alpha_mu_samples", "%s_hERG_hill_pic50_samples.txt" % sm["drug"]))
        assert samples.shape == (100, 2)
        w = ref["%s_hERG" % sm["drug"]]
        assert abs(sm["pooled_mean"][0] - w["alpha_mean"]) < 0.12 * w["alpha_mean"] + 0.03
        assert abs(sm["pooled_mean"][2] - w["mu_mean"]) < 0.015 * w["mu_mean"] + 0.03
        # chain 0 through the text file == the CPU twin, bit for bit: two Ne groups (3 and 5 experiments) on two streams that never
        # join, three segments of 20 000 iterations each, chain-0 rows copied out asynchronously behind every segment
        from oracle import c_oracle as co
        from pyhillfit_amd import hierarchical as H
        from pyhillfit_amd.sampler import gamma_table
        shapes, scales, locs = H.prior_params()
        _, _, ex = dr.load_crumb_data(sm["drug"], "hERG")
        pk = co.PackedHierPair(ex, shapes, scales, locs)
        all_pairs = [(a, b) for a in dr.drugs for b in dr.channels]
        st = pk.init_state(np.array(sm["first_iteration"]), 0.01)
        rows = pk.advance(st, 0, T, 5, 100 * (5 + 2 * ne), gamma_table(T), seed=25, chain_id=0, problem_id=all_pairs.index((sm["drug"], "hERG")))
        assert np.array_equal(chain[0, :-1], np.array(sm["first_iteration"])) and np.array_equal(chain[1:], rows)


def test_hierarchical_cli_fused_launch_chain_files_equal_the_twin(gpu, tmp_path):
    """python PyHillFit.py --hierarchical --fused-launch on: fifteen pairs of seven launch groups (Ne = 3: 4 + 4 + 4, 2 + 2 + 2, 5 + 5 + 4; Ne = 4:
    4 + 4 + 4 + 1, 4 + 4 + 4 + 3; Ne = 5: 4 + 4 + 4 + 1 + 1, 5 + 5 + 4 + 2 + 2), three segments through ONE persistent grid per segment, chain-0 rows copied out behind every segment: chain 0
    of every pair through the text file == the CPU twin, bit for bit"""
    from oracle import c_oracle as co
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    out = str(tmp_path / "output")
    T = 3000
    summ = PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-i", str(T), "-t", "5", "--drugs", "Amiodarone,Rufinamide,Verapamil,Mibefradil,Dofetilide",
                           "--channels", "hERG,Nav1.5-peak,Kv4.3", "--num-chains", "192", "--output-root", out, "--num-APs", "50",
                           "--segment", "1000", "--fused-launch", "on"])
    assert len(summ) == 15 and H.last_kernel() == 6
    shapes, scales, locs = H.prior_params()
    all_pairs = [(a, b) for a in dr.drugs for b in dr.channels]
    kinds = set()
    for sm in summ:
        ne, drug, c = sm["num_expts"], sm["drug"], sm["channel"]
        _, _, ex = dr.load_crumb_data(drug, c)
        kinds.add(H.group_key(ex, H.ISA_SHAPES))
        f = os.path.join(out, "crumb_data", "hierarchical", drug, c, "%d_expts" % ne, "chain", "crumb_data_%s_%s_hierarchical_chain.txt" % (drug, c))
        chain = np.loadtxt(f)
        pk = co.PackedHierPair(ex, shapes, scales, locs)
        st = pk.init_state(np.array(sm["first_iteration"]), 0.01)
        rows = pk.advance(st, 0, T, 5, 100 * (5 + 2 * ne), gamma_table(T), seed=25, chain_id=0, problem_id=all_pairs.index((drug, c)))
        assert np.array_equal(chain[0, :-1], np.array(sm["first_iteration"])) and np.array_equal(chain[1:], rows), (drug, c)
    assert len(kinds) == 7, kinds


def test_hierarchical_cli_all_pairs_fused_launch_on_equals_off(gpu, tmp_path):
    """all 210 Crumb pairs (every launch group: twelve shapes in the fused grid, Ne = 6 beside it) through the command line with --fused-launch on
    and off: the same chain files byte for byte, the same pooled posterior summaries"""
    import filecmp
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    res = {}
    for mode in ("on", "off"):
        out = str(tmp_path / ("output_" + mode))
        res[mode] = (out, PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-a", "-i", "4000", "-t", "5", "--num-chains", "128",
                                          "--output-root", out, "--num-APs", "20", "--segment", "2000", "--fused-launch", mode]))
    on, off = res["on"][1], res["off"][1]
    assert len(on) == len(off) == 210
    off = {(b["drug"], b["channel"]): b for b in off}                     # (the groups, and so the summaries' order, differ between the two modes)
    for a in on:
        b = off[(a["drug"], a["channel"])]
        assert a["pooled_mean"] == b["pooled_mean"] and a["pooled_sd"] == b["pooled_sd"] and a["acceptance"] == b["acceptance"], (a["drug"], a["channel"])
        rel = os.path.join("crumb_data", "hierarchical", a["drug"], a["channel"], "%d_expts" % a["num_expts"], "chain",
                           "crumb_data_%s_%s_hierarchical_chain.txt" % (a["drug"], a["channel"]))
        assert filecmp.cmp(os.path.join(res["on"][0], rel), os.path.join(res["off"][0], rel), shallow=False), rel


def test_hierarchical_cli_many_chains_without_the_fused_launch_takes_the_hipcc_kernels(gpu, tmp_path):
    """--fused-launch off with enough chains for one lane per chain: several assembly-capable groups, a launch each — they must NOT run the gfx950
    build side by side (profiles/r05/queue_progress_word_hazard.txt): every group on the hipcc kernel, no queue drained, and the same summaries as
    the fused launch gives"""
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    res = {}
    for mode in ("off", "on"):
        res[mode] = PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-a", "-i", "2000", "-t", "5", "--num-chains", "1024",
                                    "--output-root", str(tmp_path / ("out_" + mode)), "--num-APs", "10", "--segment", "1000", "--fused-launch", mode])
        assert H.last_kernel() == (1 if mode == "off" else 6), (mode, H.last_kernel())
    on = {(b["drug"], b["channel"]): b for b in res["on"]}
    assert len(res["off"]) == len(on) == 210
    for a in res["off"]:
        b = on[(a["drug"], a["channel"])]
        assert a["pooled_mean"] == b["pooled_mean"] and a["pooled_sd"] == b["pooled_sd"] and a["acceptance"] == b["acceptance"], (a["drug"], a["channel"])


def test_generic_ne_kernel_bit_identical_to_cpu_twin(gpu, oracle_pair):
    """pairs with more than 8 experiments (the reference's synthetic set: Ne = 50, dim 105, 200 points) run one wavefront per
    chain (state in LDS, lanes = experiments / factor rows): same bits as the twin across a launch cut, and the moments it
    accumulates on the device are the sums of the rows it saved; two problems of the same pair in one launch"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    p = oracle_pair("Lie-docaine", "Channel", "synthetic")
    packed = H.PackedHierPoints([p.experiments])
    ne = packed.n_expts
    assert ne == 50
    d = 5 + 2 * ne
    theta0 = np.concatenate([[1., 5., 4., .3], np.tile([4.0, 1.0], ne), [6.0]])
    C, T, thin, adapt = 20, 90, 3, 30
    s = H.HierarchicalSampler(packed, [0, 0], C, thinning=thin, seed=42, adapt_start=adapt, problem_ids=[3, 9], chain_id_base=100, device=gpu)
    s.init(np.stack([theta0, theta0]), cov_scale=0.01)
    s.enable_moments(after_iteration=0)
    row0 = s.row0.cpu().numpy()
    chain = np.concatenate([s.advance(k).cpu().numpy() for k in (adapt + 5, T - adapt - 5)])
    state = s.state.cpu().numpy().reshape(s.S, 2, C)
    mean, var, n = s.posterior_moments()
    assert n == T // thin
    np.testing.assert_allclose(mean.cpu().numpy(), chain.mean(axis=0).transpose(1, 0, 2), rtol=1e-12, atol=1e-12)   # [d+1][Q][C]
    np.testing.assert_allclose(var.cpu().numpy(), chain.var(axis=0, ddof=1).transpose(1, 0, 2), rtol=1e-7, atol=1e-12)
    assert not np.array_equal(chain[:, 0], chain[:, 1])                     # different problem ids: different streams
    pk = co.PackedHierPair(p.experiments, shapes, scales, locs)
    gam = gamma_table(T)
    for c in (0, 7, C - 1):
        st = pk.init_state(theta0, 0.01)
        assert np.array_equal(row0[0, :, c], np.concatenate([theta0, [st[d]]]))
        rows = pk.advance(st, 0, T, thin, adapt, gam, seed=42, chain_id=100 + c, problem_id=3)
        assert np.array_equal(chain[:, 0, :, c], rows)
        assert np.array_equal(state[:, 0, c], st)
    assert np.isfinite(chain).all() and (np.diff(chain[:, 0, 0, :], axis=0) != 0).any()


def _hier_posteriors_against_reference_loop(gpu, dr, fixture, C, seed, report_name, failures=None, first_experiments=False):
    """every pair of a G10-style fixture: C chains from the fixture's start point, the reference's run length and burn-in, moments on
    the device; EVERY column's pooled mean within 1 % + 4 standard errors of the reference's (the larger of: batch means pooled over the
    seeds, scatter between the seeds), every pooled sd within 20 % + 4 standard errors of the reference's OWN pooled sd — the same form as
    the bar on the means.  That standard error comes from the seeds themselves: seed i contributes V_i = sd_i^2 + (mean_i - mean)^2 to the
    pooled variance, so the pooled sd is known to r = std(V_i) / sqrt(n) / (2 mean(V_i)).  For a chain that mixes r ~ 0.01 and the band is
    [0.8, 1.2]; where each reference chain sits in its own corner of a flat direction (a steep experiment's Hill_i) or a rarely visited
    region carries part of the variance (Dofetilide-Cav1.2: 5 % of 512 GPU chains visit a low-pIC50_1 region that ten reference chains
    have not sampled in proportion; the MEDIAN chain's width is the reference's) r reaches 0.1 .. 0.2 —, acceptance within 0.02.  Returns the per-pair report.  failures: None =
    assert pair by pair; a list = collect (pair, what) of everything outside instead, so that a big fixture reports ALL of it at once.
    first_experiments (G11): an entry's pair is cut to its first e["Ne"] experiments, as the command line's -Ne does (PyHillFit.py:228-231)."""
    from pyhillfit_amd import hierarchical as H
    beyond_plain_band, columns_seen = [], [0]
    groups = {}
    for e in fixture:
        groups.setdefault(e["Ne"], []).append(e)
    report = []
    for ne, entries in sorted(groups.items()):
        T, thin = entries[0]["iterations"], entries[0]["thinning"]
        assert all(e["iterations"] == T and e["thinning"] == thin for e in entries) and T >= 300000
        exs = [dr.load_crumb_data(e["drug"], e["channel"])[2] for e in entries]
        if first_experiments:
            exs = [x[:ne] for x in exs]
        assert all(len(x) == ne for x in exs)
        s = H.HierarchicalSampler(H.PackedHierPoints(exs), list(range(len(exs))), C, thinning=thin, seed=seed, device=gpu)
        s.init(np.array([e["first_iteration"] for e in entries]), cov_scale=0.01)                   # PyHillFit.py:431
        burn_rows = (T // thin + 1) // 4                                                            # :467-471
        s.enable_moments(after_iteration=burn_rows * thin - 1)
        for _ in range(10):
            s.advance(T // 10, save=False)
        mean, var, n = s.posterior_moments()
        assert n == T // thin + 1 - burn_rows
        pooled = mean.mean(dim=2).cpu().numpy()                                                     # [dim+1][Q]
        pooled_sd = torch.sqrt(var.mean(dim=2) + mean.var(dim=2)).cpu().numpy()
        acc = s.acceptance().mean(dim=1).cpu().numpy()
        for q, e in enumerate(entries):
            p = e["pooled"]
            columns_seen[0] += len(p["mean"])
            want, want_sd = np.array(p["mean"]), np.array(p["sd"])
            se = np.maximum(p["se_batch_means"], p["se_between_seeds"])
            ratio = np.abs(pooled[:, q] - want) / (0.01 * np.abs(want) + 4 * se)
            sd_ratio = pooled_sd[:, q] / want_sd
            run_means = np.array([r["mean"] for r in e["runs"]]); run_sds = np.array([r["sd"] for r in e["runs"]])
            v_seed = run_sds ** 2 + (run_means - run_means.mean(axis=0)) ** 2                       # each seed's share of the pooled variance
            rel_se_sd = v_seed.std(axis=0, ddof=1) / np.sqrt(len(e["runs"])) / (2.0 * np.maximum(v_seed.mean(axis=0), 1e-300))
            # the band widens with the reference's OWN uncertainty about its width, but never beyond the round-3 bounds [0.5, 3.0]: with two
            # reference seeds r can reach 0.5, and an unclamped [0.8 - 4 r, 1.2 + 4 r] would make the check vacuous exactly where the
            # reference's two chains disagree
            sd_lo, sd_hi = np.maximum(0.5, 0.8 - 4 * rel_se_sd), np.minimum(3.0, 1.2 + 4 * rel_se_sd)
            beyond_plain_band.append(int(np.sum((sd_ratio <= 0.8) | (sd_ratio >= 1.2))))
            ref_acc = float(np.mean([r["acceptance"] for r in e["runs"]]))
            report.append((e["drug"], e["channel"], ne, float(ratio.max()), int(ratio.argmax()), float(sd_ratio.min()), float(sd_ratio.max()), float(acc[q])))
            print("%s %s-%s Ne=%d: worst mean ratio %.2f (column %d), sd ratios %.3f..%.3f, acceptance %.3f (reference %.3f)"
                  % ((report_name,) + report[-1] + (ref_acc,)))
            if failures is not None:
                if not ratio.max() < 1.0:
                    failures.append((e["drug"], e["channel"], "mean of column %d: ratio %.2f (GPU %.5g, reference %.5g +- %.2g)"
                                     % (int(ratio.argmax()), ratio.max(), pooled[int(ratio.argmax()), q], want[int(ratio.argmax())], se[int(ratio.argmax())])))
                if not (np.all(sd_ratio > sd_lo) and np.all(sd_ratio < sd_hi)):
                    failures.append((e["drug"], e["channel"], "sd ratios %.3f..%.3f (band of the worst column %.2f..%.2f)"
                                     % (sd_ratio.min(), sd_ratio.max(), sd_lo[int(np.argmax(sd_ratio - sd_hi))], sd_hi[int(np.argmax(sd_ratio - sd_hi))])))
                elif not (sd_ratio.min() > 0.8 and sd_ratio.max() < 1.2):
                    print("   width beyond the plain [0.8, 1.2] band, inside the reference's own uncertainty: %s-%s sd ratios %.3f..%.3f" % (e["drug"], e["channel"], sd_ratio.min(), sd_ratio.max()))
                if not abs(acc[q] - ref_acc) < 0.02:
                    failures.append((e["drug"], e["channel"], "acceptance %.3f against %.3f" % (acc[q], ref_acc)))
                continue
            assert ratio.max() < 1.0, (e["drug"], e["channel"], int(ratio.argmax()), pooled[:, q], want, se)
            assert np.all(sd_ratio > sd_lo) and np.all(sd_ratio < sd_hi), (e["drug"], e["channel"], sd_ratio, sd_lo, sd_hi)
            assert abs(acc[q] - ref_acc) < 0.02
    # a systematic width error cannot hide behind noisy two-seed bands: at most 3 % of the (pair, column) entries may lie outside the
    # PLAIN [0.8, 1.2] band at all (round 4 observed: G10 0, G10b 2 of 396, G10c/d 7 of 2 300)
    n_beyond = int(sum(beyond_plain_band))
    print("%s: %d of %d (pair, column) widths outside the plain [0.8, 1.2] band" % (report_name, n_beyond, columns_seen[0]))
    assert n_beyond <= 0.03 * columns_seen[0], (n_beyond, columns_seen[0])
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    with open(os.path.join(REPO, "gpurun_out", report_name + "_report.json"), "w") as f:
        json.dump(report, f)
    return report


def test_hierarchical_posterior_of_every_column_matches_the_reference_loop(gpu, dr_setup):
    """Golden G10 (tests/golden/make_golden_posteriors_hier.py): the reference's OWN hierarchical loop (python/PyHillFit.py:431-511
    with the target :173-193, lifted statement by statement) run at its default length — 500 000 iterations, thinning 5, first
    quarter of the saved rows dropped — with four seeds on one pair of every Ne (3, 4, 5, 6) and two weakly informative pairs.
    Here: 1 024 chains per pair from the same start point, same length, same burn-in, moments on the device.  EVERY column of the
    chain — alpha, beta, mu, s, each pIC50_i and Hill_i, sigma and the log-target — has its pooled mean within 1 % of the
    reference's + 4 of its standard errors (the larger of: batch means pooled over the seeds, scatter between the seeds), and its
    pooled sd within 20 %."""
    with open(os.path.join(GOLDEN, "g10_hier_posteriors.json")) as f:
        g10 = json.load(f)
    assert sorted(e["Ne"] for e in g10) == [3, 3, 4, 5, 6, 6]
    _hier_posteriors_against_reference_loop(gpu, dr_setup, g10, 1024, 2024, "g10")


def test_hierarchical_posterior_of_one_pair_per_drug_matches_the_reference_loop(gpu, dr_setup):
    """Golden G10b (make_golden_posteriors_hier.py --per-drug, round 4): the same lifted reference loop on ONE PAIR OF EVERY DRUG — 30
    pairs fixed by a rule written into the generator before any GPU number was seen (drug i takes channel i mod 7), two seeds each,
    500 000 iterations.  Same strict bar as G10 on every one of the 12..16 columns of every pair: with G10 that is 36 of the 210 pairs
    pinned column by column to the reference's own sampler; the other 174 rest on (alpha, mu) against the reference's stored draws
    (next test)."""
    with open(os.path.join(GOLDEN, "g10b_hier_posteriors_per_drug.json")) as f:
        g10b = json.load(f)
    assert len(g10b) == 30 and len({e["drug"] for e in g10b}) == 30 and all(len(e["runs"]) == 2 for e in g10b)
    _hier_posteriors_against_reference_loop(gpu, dr_setup, g10b, 512, 2025, "g10b")


def test_hierarchical_posterior_of_every_remaining_pair_matches_the_reference_loop(gpu, dr_setup):
    """Golden G10c (make_golden_posteriors_hier.py --all-remaining, round 4): the lifted reference loop on EVERY pair that is in neither
    G10 nor G10b, two seeds each (301, 302; rule fixed in the generator before any run existed).  With G10 and G10b every one of the
    210 Crumb pairs then has every column of its hierarchical chain pinned to the reference's own sampler under the same strict bar.
    (The fixture holds the pairs whose two runs are complete; the generation takes ~4 hours of 7 cores and can be resumed.)"""
    path = os.path.join(GOLDEN, "g10c_hier_posteriors_all_remaining.json")
    if not os.path.exists(path):
        pytest.skip("fixture not generated (tests/golden/make_golden_posteriors_hier.py --all-remaining)")
    with open(path) as f:
        g10c = json.load(f)
    with open(os.path.join(GOLDEN, "g10_hier_posteriors.json")) as f:
        pinned = {(e["drug"], e["channel"]) for e in json.load(f)}
    with open(os.path.join(GOLDEN, "g10b_hier_posteriors_per_drug.json")) as f:
        pinned |= {(e["drug"], e["channel"]) for e in json.load(f)}
    mine = [(e["drug"], e["channel"]) for e in g10c]
    assert len(mine) >= 1 and len(set(mine)) == len(mine) and not (set(mine) & pinned)
    assert all([r["seed"] for r in e["runs"]] == [301, 302] for e in g10c)
    # G10d: the follow-up of the eight pairs whose first comparison had an entry outside the bar (a steep experiment's Hill_i in the heavy
    # tail of the log-logistic level: the reference's own two chains disagree by up to 55 of their standard errors there) — eight further
    # seeds each, pooled with the two: ten reference chains, whose scatter says how well the reference itself knows such a mean
    path_d = os.path.join(GOLDEN, "g10d_hier_posteriors_follow_up.json")
    followed = []
    if os.path.exists(path_d):
        with open(path_d) as f:
            g10d = {(e["drug"], e["channel"]): e for e in json.load(f)}
        for e in g10c:
            d = g10d.get((e["drug"], e["channel"]))
            if d is None:
                continue
            runs = e["runs"] + d["runs"]
            means = np.array([r["mean"] for r in runs]); sds = np.array([r["sd"] for r in runs]); ses = np.array([r["batch_means_se"] for r in runs])
            n = len(runs)
            assert n == 10 and e["first_iteration"] == d["first_iteration"]
            e["runs"] = runs
            e["pooled"] = {"mean": means.mean(axis=0).tolist(), "sd": np.sqrt((sds ** 2).mean(axis=0) + means.var(axis=0)).tolist(),
                           "se_batch_means": (np.sqrt((ses ** 2).sum(axis=0)) / n).tolist(),
                           "se_between_seeds": (means.std(axis=0, ddof=1) / np.sqrt(n)).tolist()}
            followed.append((e["drug"], e["channel"]))
    failures = []
    report = _hier_posteriors_against_reference_loop(gpu, dr_setup, g10c, 512, 2026, "g10c", failures=failures)
    print("G10c: %d pairs (+ %d in G10 / G10b = %d of 210 pinned column by column; %d of them against ten reference seeds: %s); worst mean ratio %.2f; outside the bar: %s"
          % (len(mine), len(pinned), len(mine) + len(pinned), len(followed), followed, max(r[3] for r in report), failures))
    assert not failures, failures                                   # no pair, no column excepted


def test_g10e_replication_of_the_widest_pairs_against_48_fresh_reference_seeds(gpu, dr_setup):
    """Golden G10e (make_golden_posteriors_hier.py --replication; rule AND this test committed before any of its runs existed): the three
    pairs whose GPU width still lay beyond the plain [0.8, 1.2] band against their ten reference seeds in round 4 — 48 FRESH seeds each
    (401..448), a GPU seed not used before, the 48 seeds ALONE, the helper's bar exactly as it stands (mean 1 % + 4 s.e., sd 20 % + 4 s.e. of
    the reference's pooled sd — ~2.2 x narrower with 48 seeds than with ten —, acceptance 0.02, and its fixture-level clause: at most 3 % of the
    (pair, column) entries beyond the plain band).  No pair, no column excepted; nothing is topped up."""
    path = os.path.join(GOLDEN, "g10e_hier_posteriors_replication.json")
    if not os.path.exists(path):
        pytest.skip("fixture not generated (tests/golden/make_golden_posteriors_hier.py --replication)")
    with open(path) as f:
        g10e = json.load(f)
    if len(g10e) < 3:
        pytest.skip("fixture incomplete: the generation (144 reference runs) writes it pair by pair; the comparison is defined on all three pairs")
    assert [(e["drug"], e["channel"]) for e in g10e] == [("Azithromycin", "Kir2.1"), ("Ranolazine", "Cav1.2"), ("Dofetilide", "Cav1.2")]
    assert all([r["seed"] for r in e["runs"]] == list(range(401, 449)) for e in g10e)
    failures = []
    _hier_posteriors_against_reference_loop(gpu, dr_setup, g10e, 512, 2027, "g10e", failures=failures)
    assert not failures, failures


def test_all_pairs_alpha_mu_against_the_reference_stored_samples(gpu):
    """every Crumb pair at the reference's run length (500 000 iterations, first quarter dropped), 128 chains each: pooled
    posterior means of (alpha, mu) against the reference's own stored hierarchical samples (chaste/samples: 500 draws of ONE
    unseeded chain per pair, so each reference mean carries a Monte-Carlo error of a few sd/sqrt(500)).  Observed: all 210
    pairs within 3.3 such errors.  (Shorter runs do NOT agree for the weakly informative pairs: their chains need well over
    60 000 iterations to leave the start point — which is why the reference runs 500 000.)"""
    from pyhillfit_amd import bestfit
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    with open(os.path.join(GOLDEN, "chaste_alpha_mu_stats.json")) as f:
        ref = json.load(f)
    shapes, scales, locs = H.prior_params()
    groups = {}
    for d in dr.drugs:
        for c in dr.channels:
            ne, _, ex = dr.load_crumb_data(d, c)
            groups.setdefault(len(ex), []).append((d, c, ex))
    T, C = 500000, 128
    z, names, sd_ratio = [], [], []
    for ne, members in sorted(groups.items(), reverse=True):
        packed = H.PackedHierPoints([m[2] for m in members])
        theta0 = np.array([bestfit.hierarchical_first_iteration(m[2], locs) for m in members])
        s = H.HierarchicalSampler(packed, list(range(len(members))), C, thinning=5, seed=7, device=gpu)
        s.init(theta0, cov_scale=0.01)
        s.enable_moments(after_iteration=T // 4)
        s.advance(T, save=False)
        mean, var, n = s.posterior_moments()
        pooled = mean.mean(dim=2).cpu().numpy()                      # [dim+1][Q]
        pooled_sd = torch.sqrt(var.mean(dim=2) + mean.var(dim=2)).cpu().numpy()
        for q, (d, c, _) in enumerate(members):
            w = ref["%s_%s" % (d.replace("/", "_"), c.replace("/", "_"))]
            se_a, se_m = 3 * w["alpha_sd"] / np.sqrt(w["n"]), 3 * w["mu_sd"] / np.sqrt(w["n"])    # x3: autocorrelated draws
            z.append(max(abs(pooled[0, q] - w["alpha_mean"]) / (se_a + 0.005 * w["alpha_mean"]),
                         abs(pooled[2, q] - w["mu_mean"]) / (se_m + 0.005 * abs(w["mu_mean"]))))
            sd_ratio.append((pooled_sd[0, q] / w["alpha_sd"], pooled_sd[2, q] / w["mu_sd"]))
            names.append((d, c))
    z, sd_ratio = np.array(z), np.array(sd_ratio)
    assert len(names) == 210
    print("chaste/samples: worst z %.2f at %s; pairs beyond 3: %s" % (z.max(), names[int(z.argmax())], [(names[k], round(float(z[k]), 2)) for k in np.flatnonzero(z > 3)]))
    assert z.max() < 4, (names[int(z.argmax())], z.max(), [(names[k], float(z[k])) for k in np.flatnonzero(z >= 4)])       # no pair allowed outside (round 4: was max < 6 and 98 % below 4)
    assert np.all(sd_ratio > 0.6) and np.all(sd_ratio < 1.6), (sd_ratio.min(), sd_ratio.max())   # posterior widths too
