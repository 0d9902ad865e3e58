"""Replica exchange between ladder rungs on the GPU (phf_replica_exchange_*): one swap round against a numpy restatement, the
Delta t = 0 known answer, cut invariance, a host replay of 50 rounds, the stepping-stone se over replica sets, the G6 known answer
by quadrature with swaps, and the command lines."""
import json
import math
import os

import numpy as np
import pytest

from conftest import REPO
from test_gpu_stepping_stone import G6_PAIRS, pair_data, tempered_sampler
from test_math_philox import philox_python

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RX_DOMAIN = 0x40000000
SEEN_BOTTOM, HEADING_DOWN = 1 << 30, 1 << 29


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


def sampler_for(dr, pairs, model, temps, chains, device, thinning=5, seed=1, iterations=100000):
    """a tempered sampler over pairs x the given rung temperatures (pair-major), problem ids 0..Q-1"""
    from pyhillfit_amd.sampler import SingleLevelSampler
    d = model + 1
    R = len(temps)
    packed = dr.PackedPoints([pair_data(dr, a, b) for a, b in pairs])
    pair_index = np.repeat(np.arange(len(pairs)), R)
    s = SingleLevelSampler(packed, model, pair_index, np.tile(temps, len(pairs)), chains, thinning=thinning, seed=seed,
                           adapt_start=1000 * d, reset_mean_at_adapt_start=True, problem_ids=np.arange(len(pair_index)), device=device)
    s.init(np.ones(d), cov_identity=True, cov_scale=1.0)
    s.enable_moments(after_iteration=0)
    s.reserve(iterations)
    return s, packed, pair_index


def u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) * 2.0 ** -53


def arrive(label, rung, R):
    """the label of a replica arriving at `rung`, and whether it completed a round trip 0 -> R-1 -> 0"""
    trip = False
    if rung == R - 1 and label & SEEN_BOTTOM:
        label |= HEADING_DOWN
    if rung == 0:
        trip = bool(label & HEADING_DOWN)
        label = (label & ~HEADING_DOWN) | SEEN_BOTTOM
    return label, trip


def numpy_round(state, labels, trips, s, temps_q, pids, R, C, seed, model, prior_of, log_of, decide=None):
    """one swap round in numpy on host copies (state [S][Q*C], labels [Q*C], trips [P][C]), in place.
    decide(p, k, c, u, log_u, log_alpha) -> bool overrides the decision (default: log_u < log_alpha).  prior_of(theta [n][d]) and
    log_of(u [n]) evaluate the prior and log u.  Returns (u, log u, log alpha, decision) arrays [P][R-1][C] (NaN where not proposed)
    and accepts [P][R-1]."""
    d = model + 1
    LL = state.shape[0] - 1
    P = len(temps_q) // R
    parity = s & 1
    ks = list(range(parity, R - 1, 2))
    U = np.full((P, R - 1, C), np.nan); LU = U.copy(); LA = U.copy(); DEC = np.zeros((P, R - 1, C), dtype=bool)
    lanes = []
    for p in range(P):
        for k in ks:
            qa = p * R + k
            for c in range(C):
                w = philox_python([c, int(pids[qa]), s, RX_DOMAIN, seed & 0xffffffff, seed >> 32], 7)
                U[p, k, c] = u53(w[0], w[1])
                lanes.append((p, k, c))
    pp, kk, cc = (np.array(v) for v in zip(*lanes))
    lu = log_of(U[pp, kk, cc])
    LU[pp, kk, cc] = lu
    qa = pp * R + kk
    ga, gb = qa * C + cc, (qa + 1) * C + cc
    with np.errstate(invalid="ignore"):
        la = (temps_q[qa + 1] - temps_q[qa]) * (state[LL, ga] - state[LL, gb])
    LA[pp, kk, cc] = la
    dec = np.array([decide(p, k, c, U[p, k, c], LU[p, k, c], LA[p, k, c]) if decide else bool(LU[p, k, c] < LA[p, k, c])
                    for p, k, c in lanes], dtype=bool)
    DEC[pp, kk, cc] = dec
    a, b = ga[dec], gb[dec]
    th_a, th_b = state[:d, a].copy(), state[:d, b].copy()
    ll_a, ll_b = state[LL, a].copy(), state[LL, b].copy()
    ta, tb = temps_q[qa[dec]], temps_q[qa[dec] + 1]
    with np.errstate(invalid="ignore"):
        lik_a = np.where(ta == 0.0, 0.0, ta * ll_b)
        lik_b = np.where(tb == 0.0, 0.0, tb * ll_a)
    state[:d, a], state[:d, b] = th_b, th_a
    state[LL, a], state[LL, b] = ll_b, ll_a
    state[d, a] = lik_a + prior_of(th_b.T)
    state[d, b] = lik_b + prior_of(th_a.T)
    for i, (ia, ib) in enumerate(zip(a, b)):
        k = int(kk[dec][i]); p = int(pp[dec][i]); c = int(cc[dec][i])
        lab_a, trip = arrive(int(labels[ib]), k, R)
        lab_b, _ = arrive(int(labels[ia]), k + 1, R)
        labels[ia], labels[ib] = lab_a, lab_b
        trips[p, c] += trip
    accepts = DEC.sum(axis=2)
    return U, LU, LA, DEC, accepts, ks


def prior_fn(packed, model, device):
    from pyhillfit_amd.sampler import log_target_batch

    def prior_of(theta):
        theta = np.atleast_2d(theta)
        if theta.shape[0] == 0:
            return np.zeros(0)
        _, pri = log_target_batch(packed, model, np.zeros(len(theta), dtype=np.int32), np.zeros(len(theta)), theta, device)
        return pri
    return prior_of


def log_fn(device):
    from pyhillfit_amd.sampler import debug_math
    return lambda u: debug_math(10, u, device) if len(u) else np.zeros(0)      # phf_log_fast_k: the kernel's log u


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit-identical, except that any NaN equals any NaN (the device's NaN has another sign and payload than numpy's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


@pytest.mark.parametrize("model", [1, 2])
def test_swap_round_matches_numpy(gpu, dr_setup, model):
    """3 pairs x 6 rungs (one at t = 0) x 128 chains of random states, some l = -inf or NaN; an odd and an even round"""
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    dr = dr_setup
    temps = np.array([0.0, 0.01, 0.1, 0.35, 0.7, 1.0])
    pairs = [("Amiodarone", "hERG"), ("Bepridil", "Kv4.3"), ("Quinidine", "Nav1.5-peak")]
    R, C, d = len(temps), 128, model + 1
    s, packed, pair_index = sampler_for(dr, pairs, model, temps, C, gpu, seed=0x123456789)
    rx = ReplicaExchange(s, R)
    rng = np.random.default_rng(40 + model)
    S, N = s.state.shape
    st = rng.normal(size=(S, N))
    st[0] = rng.uniform(-4.0, 9.0, N)
    if model == 2:
        st[1] = rng.uniform(-0.5, 11.0, N)
    st[d - 1] = rng.uniform(-0.01, 20.0, N)                                # sigma
    ll = rng.normal(-100.0, 60.0, N)
    ll[rng.random(N) < 0.05] = -np.inf
    ll[rng.random(N) < 0.03] = np.nan
    st[S - 1] = ll
    st[d] = rng.normal(-50, 10, N)
    s.state.copy_(torch.from_numpy(st))
    lab0 = (np.repeat(np.arange(len(pairs) * R) % R, C) | (rng.integers(0, 4, N) << 29)).astype(np.int32)
    rx.labels.copy_(torch.from_numpy(lab0))
    temps_q = np.tile(temps, len(pairs))
    prior_of, log_of = prior_fn(packed, model, gpu), log_fn(gpu)
    host, labels, trips = st.copy(), lab0.copy(), np.zeros((len(pairs), C), dtype=np.int64)
    att_sum = np.zeros((len(pairs), R - 1), dtype=np.int64); acc_sum = att_sum.copy()
    for rnd in (7, 8):
        trace = torch.full((len(pairs), R - 1, C, 3), np.nan, dtype=torch.float64, device=gpu)
        rx.swap_round(rnd, trace=trace)
        tr = trace.cpu().numpy()
        dev_dec = tr[..., 1] < tr[..., 2]

        def decide(p, k, c, u, lu, la):
            return bool(dev_dec[p, k, c])
        U, LU, LA, DEC, accepts, ks = numpy_round(host, labels, trips, rnd, temps_q, np.arange(len(temps_q)), R, C, 0x123456789, model,
                                                  prior_of, log_of, decide)
        prop = ~np.isnan(U)
        assert prop.sum() == len(pairs) * len(ks) * C and np.isnan(tr[..., 0][~prop]).all()
        assert np.array_equal(bits(tr[..., 0][prop]), bits(U[prop]))                    # u: Philox + phf_uniform53, bit for bit
        with np.errstate(divide="ignore"):
            ref_log = np.log(U[prop])
        assert np.all(np.abs(tr[..., 1][prop] - ref_log) <= 1e-15 * np.abs(ref_log))
        assert same(tr[..., 2][prop], LA[prop])                                          # log alpha: the same IEEE operations
        with np.errstate(invalid="ignore"):
            np_dec = ref_log < LA[prop]
            far = np.abs(ref_log - LA[prop]) > 1e-12
        assert np.array_equal(dev_dec[prop][far], np_dec[far])
        assert np.all(~dev_dec[prop][np.isnan(LA[prop])])                                # NaN rejects
        att_sum[:, ks] += C
        acc_sum += accepts
        got = s.state.cpu().numpy()
        assert same(got, host), np.argwhere(bits(got) != bits(host))[:5]
        assert np.array_equal(rx.labels.cpu().numpy(), labels)
        stt = rx.statistics()
        assert np.array_equal(stt["attempts"], att_sum) and np.array_equal(stt["accepts"], acc_sum)
        assert np.array_equal(stt["round_trips"], trips)
        print("round %d: %d of %d proposals accepted" % (rnd, int(DEC.sum()), int(prop.sum())))
    assert acc_sum.sum() > 0 and acc_sum.sum() < att_sum.sum() and trips.sum() >= 0


def test_equal_temperatures_swap_everything(gpu, dr_setup):
    """Delta t = 0: log alpha = 0 > log u, every proposal is accepted and one round exchanges the two slots exactly"""
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    s, packed, _ = sampler_for(dr_setup, [("Amiodarone", "hERG")], 2, np.array([0.5, 0.5]), 64, gpu)
    s.advance(300, save=False)
    rx = ReplicaExchange(s, 2)
    before = s.state.cpu().numpy().reshape(s.S, 2, 64)
    assert np.isfinite(before[-1]).all()
    rx.swap_round(2)
    after = s.state.cpu().numpy().reshape(s.S, 2, 64)
    moved = list(range(4)) + [s.S - 1]                                   # theta, log-target, l
    assert np.array_equal(bits(after[moved][:, 0]), bits(before[moved][:, 1]))
    assert np.array_equal(bits(after[moved][:, 1]), bits(before[moved][:, 0]))
    stay = [f for f in range(s.S) if f not in moved]
    assert np.array_equal(bits(after[stay]), bits(before[stay]))
    st = rx.statistics()
    assert st["attempts"].tolist() == [[64]] and st["accepts"].tolist() == [[64]]
    assert (rx.replicas() == np.array([[1] * 64, [0] * 64])).all()
    assert st["round_trips"].sum() == 0                                  # the replica from rung 1 never visited rung 0 before


def run_cut(dr, cuts, device, K=3, thin=5):
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    t = dr.temperature_ladder(3)
    s, _, _ = sampler_for(dr, [("Amiodarone", "hERG"), ("Quinidine", "Nav1.5-peak")], 2, t, 64, device, thinning=thin)
    rx = ReplicaExchange(s, len(t))
    rows = []
    for n in cuts:
        rows.append(rx.advance(n, every=K))
    return torch.cat(rows).cpu().numpy(), s, rx


def test_cut_invariance(gpu, dr_setup):
    K, T = 3, 600
    one, s1, rx1 = run_cut(dr_setup, [T], gpu, K)
    cut, s2, rx2 = run_cut(dr_setup, [7 * K, 13 * K + 3, T - 20 * K - 3], gpu, K)
    assert one.shape == cut.shape == (T // 5, 8, 4, 64)
    assert np.array_equal(bits(one), bits(cut))
    assert np.array_equal(bits(s1.state.cpu().numpy()), bits(s2.state.cpu().numpy()))
    assert np.array_equal(bits(s1.moments.cpu().numpy()), bits(s2.moments.cpu().numpy()))
    assert np.array_equal(rx1.labels.cpu().numpy(), rx2.labels.cpu().numpy())
    a, b = rx1.statistics(), rx2.statistics()
    assert all(np.array_equal(a[k], b[k]) for k in a) and rx1.rounds == rx2.rounds == T // K
    assert a["accepts"].sum() > 0
    # and a checkpoint continues bit-identically
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    sd, rsd = s1.state_dict(), rx1.state_dict()
    more1 = rx1.advance(30, every=K).cpu().numpy()
    s1.load_state_dict(sd)
    rx3 = ReplicaExchange(s1, rx1.R)
    rx3.load_state_dict(rsd)
    more3 = rx3.advance(30, every=K).cpu().numpy()
    assert np.array_equal(bits(more1), bits(more3))


def test_host_replay_of_50_rounds(gpu, dr_setup):
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    dr = dr_setup
    K, rounds, model, C = 4, 50, 2, 64
    t = dr.temperature_ladder(4)
    pairs = [("Amiodarone", "hERG"), ("Bepridil", "Kv4.3")]
    dev_s, packed, _ = sampler_for(dr, pairs, model, t, C, gpu)
    rx = ReplicaExchange(dev_s, len(t))
    rx.advance(K * rounds, every=K, save=False)
    host_s, _, _ = sampler_for(dr, pairs, model, t, C, gpu)
    R = len(t)
    labels = np.repeat(np.arange(len(pairs) * R) % R, C).astype(np.int32)
    labels[np.repeat(np.arange(len(pairs) * R) % R, C) == 0] |= SEEN_BOTTOM
    trips = np.zeros((len(pairs), C), dtype=np.int64)
    acc = np.zeros((len(pairs), R - 1), dtype=np.int64)
    prior_of, log_of = prior_fn(packed, model, gpu), log_fn(gpu)
    temps_q = np.tile(t, len(pairs))
    for r in range(1, rounds + 1):
        host_s.advance(K, save=False)
        st = host_s.state.cpu().numpy()
        acc += numpy_round(st, labels, trips, r, temps_q, np.arange(len(temps_q)), R, C, host_s.seed, model, prior_of, log_of)[4]
        host_s.state.copy_(torch.from_numpy(st))
    assert np.array_equal(bits(dev_s.state.cpu().numpy()), bits(host_s.state.cpu().numpy()))
    assert np.array_equal(bits(dev_s.moments.cpu().numpy()), bits(host_s.moments.cpu().numpy()))
    assert np.array_equal(rx.labels.cpu().numpy(), labels)
    stt = rx.statistics()
    assert np.array_equal(stt["accepts"], acc) and np.array_equal(stt["round_trips"], trips)
    print("replay: %d swaps accepted over %d rounds, %d round trips" % (int(acc.sum()), rounds, int(trips.sum())))


def test_se_joint_matches_numpy(gpu, dr_setup):
    from pyhillfit_amd import replica_exchange as rxm
    from pyhillfit_amd import stepping_stone as ss
    dr = dr_setup
    t = dr.temperature_ladder(5)
    R, C, thin = len(t), 128, 5
    s, packed, pair_index = sampler_for(dr, G6_PAIRS, 1, t, C, gpu, thinning=thin)
    rx = rxm.ReplicaExchange(s, R)
    rows = rx.advance(3000, every=10)[100:].contiguous()
    st = ss.SteppingStone(packed, 1, pair_index, np.tile(ss.deltas(t), 2), C, rows.shape[0], gpu)
    st.accumulate(rows)
    got = rxm.joint_se(st, 2, R)
    want = rxm.joint_se_numpy(st.accumulators(), st.reduced()[:, 0], 2, R)
    print("se over replica sets", got, want)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    np.testing.assert_allclose(got, want, rtol=1e-12)


# ---- known answer by quadrature with swaps (the G6 setup) ----------------------------------------------------------------------
def g6_case(dr, model, K, T, device):
    """the G6 setup (41 rungs, 256 chains, thinning 5, burn-in 1/4) with swaps every K iterations for T iterations: one printed line
    and the rule's two verdicts (SS, TI) per pair"""
    from pyhillfit_amd import replica_exchange as rxm
    from pyhillfit_amd import stepping_stone as ss
    with open(os.path.join(REPO, "profiles", "stepping_stone", "exact_ladder_by_quadrature.json")) as f:
        exact = json.load(f)
    thin, C = 5, 256
    s, packed, pair_index, t, num_saved, burn = tempered_sampler(dr, G6_PAIRS, model, None, C, T, thin, device)
    R, Q, d = len(t), len(pair_index), model + 1
    rx = rxm.ReplicaExchange(s, R)
    st = ss.SteppingStone(packed, model, pair_index, np.tile(ss.deltas(t), len(G6_PAIRS)), C, num_saved - burn, device)
    seg = 5000
    buf = torch.empty((seg // thin, Q, d + 1, C), dtype=torch.float64, device=device)
    done, r = 0, 1
    while done < T:
        k = min(seg, T - done)
        nr = k // thin
        rows = rx.advance(k, every=K, out=buf[:nr])
        first = max(0, burn - r)
        if first < nr:
            st.accumulate(rows[first:])
        done += k; r += nr
    red = st.reduced()
    se_joint = rxm.joint_se(st, len(G6_PAIRS), R)
    ll1 = s.mean_log_likelihood_t1().cpu().numpy()
    se_ti = rxm.replica_set_ti_se(ll1, t, len(G6_PAIRS))
    stats = rx.statistics()
    lines, verdicts = [], []
    for ip, (drug, channel) in enumerate(G6_PAIRS):
        ex = exact["%s|%s|%d" % (drug, channel, model)]
        u = slice(ip * R, (ip + 1) * R)
        log_z_ss = float(np.sum(red[u, 0][:-1]))
        ti = float(dr.trapezium_rule(t, ll1[u].mean(axis=1)))
        ti_target = ex["log_z"] + ex["ladder_bias"]
        z = (red[u, 0][:-1] - np.asarray(ex["log_r"])[:R - 1]) / red[u, 1][:-1]
        worst = np.argsort(-np.abs(z))[:3]
        rate = stats["accepts"][ip] / np.maximum(stats["attempts"][ip], 1)
        lines.append("%s + %s model %d, swaps every %d, %d iterations: log Z %.5f, SS %.5f +- %.5f (SS - exact %+.5f), TI %.5f +- %.5f "
                     "(TI - (log Z + ladder bias) %+.5f); lowest accept rate %.3f at rungs %d-%d; round trips per replica set %.2f; "
                     "worst rungs %s"
                     % (drug, channel, model, K, T, ex["log_z"], log_z_ss, se_joint[ip], log_z_ss - ex["log_z"], ti, se_ti[ip],
                        ti - ti_target, rate.min(), int(rate.argmin()), int(rate.argmin()) + 1, stats["round_trips"][ip].mean(),
                        ["k %d t %.4f z %+.1f" % (k, t[k], z[k]) for k in worst]))
        verdicts.append((abs(log_z_ss - ex["log_z"]) <= 4 * se_joint[ip] + 0.01, abs(ti - ti_target) <= 4 * se_ti[ip] + 0.01))
    return lines, verdicts


@pytest.mark.parametrize("model", [1, 2])
def test_known_answer_by_quadrature_with_swaps(gpu, dr_setup, model):
    """Rule (fixed before the first GPU run): |log Z_SS - log Z| <= 4 se_joint + 0.01 and |TI - (log Z + ladder_bias)| <= 4 se_TI + 0.01
    for both G6 pairs, with swaps every replica_exchange.RECOMMENDED_EVERY iterations; exact answers from
    profiles/stepping_stone/exact_ladder_by_quadrature.json.  At 100 000 iterations the rule fails for K = 10 and K = 5; with K = 2 and
    400 000 iterations (the fallback the rule allowed) it holds (profiles/replica_exchange/results.txt)."""
    from pyhillfit_amd import replica_exchange as rxm
    lines, verdicts = g6_case(dr_setup, model, rxm.RECOMMENDED_EVERY, 400000, gpu)
    for line in lines:
        print(line)
    assert all(a and b for a, b in verdicts), verdicts                 # every case evaluated and printed before the verdict


# ---- the command lines ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def csv_file(tmp_path_factory, gpu):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def test_cli(csv_file, tmp_path, capsys):
    from pyhillfit_amd import PyHillTemp, compute_bayes_factors
    common = ["--data-file", csv_file, "-d", "0", "-c", "0", "-i", "4000", "-t", "5", "--rungs", "4", "--num-chains", "64",
              "--stepping-stone"]
    on = str(tmp_path / "on")
    for m in ("1", "2"):
        PyHillTemp.main(common + ["-m", m, "--output-root", on, "--swap-every", "10"])
    printed = capsys.readouterr().out
    assert printed.count("replica exchange Amiodarone + hERG model") == 2
    base = os.path.join(on, "crumb_data", "single-level", "Amiodarone", "hERG")
    recs = {}
    for m in (1, 2):
        with open(os.path.join(base, "model_%d" % m, "thermodynamic_integration.json")) as f:
            ti = json.load(f)
        rx = ti["replica_exchange"]
        assert rx["every"] == 10 and rx["rounds"] == 400 and len(rx["accept_rate"]) == 4
        assert all(0.0 <= a <= 1.0 for a in rx["accept_rate"]) and rx["attempts"] == [200 * 64] * 4
        assert rx["round_trips"] >= 0 and rx["round_trips_per_replica_set"] == rx["round_trips"] / 64
        sst = recs[m] = ti["stepping_stone"]
        assert sst["se_method"] == "replica_sets" and sst["se"] > 0 and sst["se_independent_rungs"] > 0
        assert ti["expectation_se_replica_sets"] > 0
        with open(os.path.join(on, "crumb_data", "tempered_summary_model_%d.json" % m)) as f:
            summ = json.load(f)
        assert [r["swap_accept_rate"] for r in summ["rungs"]] == rx["accept_rate"] + [None]
    bf = str(tmp_path / "BFs") + "/"
    res = compute_bayes_factors.main(["--data-file", csv_file, "-d", "0", "-c", "0", "--rungs", "4", "--output-root", on, "--bf-dir", bf,
                                      "--estimator", "stepping-stone"])
    assert res["log_B12_se"] == pytest.approx(math.hypot(recs[1]["se"], recs[2]["se"]), rel=1e-12)
    assert res["se_methods"] == {1: "replica_sets", 2: "replica_sets"}
    assert "over replica sets" in capsys.readouterr().out
