"""CPU: the gated weights (tests/gated_weights.py) -- everything tests/test_gated_gpu.py relies on.  No figure in this file or in the tolerance comes from a device run.

Per size (128, 64, 32, 16), on the content gw.content generates and one float64 reference of it (computed once, shared by the tests of the size):

  zero CU      logits exactly 0.0, and every gated pre-activation of the zero CU <= -b / 2: a rounding error cannot open a gate
  fold         folding the gated state dict in float64 gives |weights| equal to the tracer's to 1e-6 relative, scales of magnitude 2^-2 .. 2^2, gamma and var both
               away from 1, 1/4 +- 1/8 of the channels negative at every gated site, folded biases -b / +b / -2 b as designed; the blob packs and round-trips
  activity     over the impulse content the bias clips 20 % .. 80 % of the light cone (the entries that are positive without the bias) at every gated site
  empty        at most 5 % of the (CU, logit) pairs have a float64 expectation of exactly 0 (twelve zero CUs of each size are among them by design)
  tolerance    gw.RHO_GATED_FAST / RHO_GATED_EXACT are recomputed (8 x the fp16 / hilo emulation's largest |error| / M over the impulse content, the exact table
               floored at 8 x gw.GATED_ORACLE_MEASURED) and the committed figures held to 2 %
  power        for every mutation (norelu, nobias, relu_before_add x the gated places) but the pairs of gw.UNSEEN -- which are held NOT to reach it, so that the
               table stays what is measured -- the float64 mutated network differs from the float64 network by more than 2 x rho_fast x M at some CU of gw.mutation_cus; against rho_exact as well for the sizes whose default arithmetic is exact (64, 32, 16).  norelu at the
               last gated site moves the zero CU off 0.0 (128, 64, 32: a head pools that site; 16: none does, every later ReLU clips the pixel again).  relu_before_add cannot: at a ".1.out" site it is relu(0 - b) + 0 = 0 on the zero CU, the same value, and
               behind a ".0.out" site, where it gives relu(+b) - 2 b = -b, every later site clips the negative pixel again -- docs/NUMERICS.md ("Gated weights")
  oracle       forward64 of the gated set agrees with the C oracle and with oracle/torch_port.py on 44 CUs per size to gw.GATED_ORACLE_MEASURED x M (fp32
               accumulation: the bound of tests/test_tracer_cpu.py, 6e-5, holds a fortiori; measured 6.7e-8 / 7.4e-8 / 1.34e-7 / 2.73e-7 for 128 / 64 / 32 / 16).  The only place the oracle is used."""
import time

import numpy as np
import pytest

import gated_weights as gw
import tracer_weights as tw

SIZES = gw.SIZES
ORACLE_BOUND = 6e-5
EXACT_BY_DEFAULT = (64, 32, 16)
_CACHE = {}


def state(size):
    """The state dict, the content, its float64 reference and M of a size, computed once."""
    if size not in _CACHE:
        t0 = time.time()
        sd = gw.gated_state_dict(tw.arch_of(size), size)
        labels, org, pred, is_zero, is_imp = gw.content(size)
        ref = gw.reference(size, org, pred, sd=sd)
        _CACHE[size] = dict(sd=sd, labels=labels, org=org, pred=pred, is_zero=is_zero, is_imp=is_imp, ref=ref, M=gw.magnitude(size, org, pred))
        print(f"size {size}: {len(org)} CUs ({len(gw.unique_rows(org, pred)[0])} distinct), float64 reference and M {time.time() - t0:.1f} s")
    return _CACHE[size]


@pytest.mark.parametrize("size", SIZES)
def test_zero_cu_and_its_gates(size):
    import torch
    st = state(size)
    assert int(st["is_zero"].sum()) == 12 and st["is_zero"][0] and st["is_zero"][-1]
    assert (st["ref"][st["is_zero"]] == 0.0).all(), "the zero CU must give logits exactly 0.0"
    assert (st["M"][st["is_zero"]] == 0.0).all() and (st["M"][~st["is_zero"]] > 0).all()
    pre = {}
    with torch.no_grad():
        gw.GatedNet(st["sd"]).forward(torch.zeros((1, 2, size, size), dtype=torch.float64), pre=pre)
    for site in gw.gated_sites(size):
        lin, bias = pre[site]
        b = gw.B[size][site]
        z = (lin + bias[None, :, None, None]).max().item()
        assert b > 0 and z <= -b / 2, (site, z, b)
        assert z == pytest.approx(-b, rel=1e-5)
    for site in set(gw.sites(tw.arch_of(size))) - set(gw.gated_sites(size)):
        assert (pre[site][0] == 0).all() and (pre[site][1] == 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_fold(pkg, size):
    arch = tw.arch_of(size)
    sd, tr = state(size)["sd"], tw.tracer_state_dict(arch)
    net, ref = gw.GatedNet(sd), gw.GatedNet(tr)
    gated = gw.gated_sites(size)
    assert len(gated) == {128: 16, 64: 12, 32: 8, 16: 4}[size]
    for (p, _, c1, c2, sc), (_, _, r1, r2, rsc) in zip(net.blocks, ref.blocks):
        for (w, _), (rw, _) in ((c1, r1), (c2, r2)) + (((sc, rsc),) if sc is not None else ()):
            assert float((np.abs(w.abs().numpy() - rw.numpy()) / rw.numpy()).max()) <= 1e-6, p
        for which, convs in (("conv1", [("bn1", c1, -1.0)]), ("out", [("bn2", c2, 1.0 if sc is not None else -1.0)] + ([("shortcut.1", sc, -2.0)] if sc is not None else []))):
            site = f"{p}.{which}"
            signs = []
            for bn, (w, bias), mult in convs:
                gamma, var = sd[f"{p}.{bn}.weight"].astype(np.float64), sd[f"{p}.{bn}.running_var"].astype(np.float64)
                s = gamma / np.sqrt(var + tw.BN_EPS)
                if site not in gated:
                    assert (gamma == 1).all() and (var == 1).all() and (bias.numpy() == 0).all() and (w.numpy() > 0).all(), site
                    continue
                e = np.log2(np.abs(s) * np.sqrt(1 + tw.BN_EPS))
                assert np.abs(e - np.rint(e)).max() < 1e-6 and set(np.rint(e).astype(int)) == {-2, -1, 0, 1, 2}, (site, bn)
                assert (np.abs(np.abs(gamma) - 1) >= 0.5).all() and (np.abs(var - 1) >= 0.7).all(), (site, bn)
                assert (sd[f"{p}.{bn}.running_mean"] != 0).all() and (sd[f"{p}.{bn}.bias"] != 0).all(), (site, bn)
                assert np.abs(bias.numpy() - mult * gw.B[size][site]).max() <= 1e-6 * gw.B[size][site], (site, bn)
                assert (np.sign(w.numpy().reshape(len(s), -1)) == np.sign(s)[:, None]).all(), (site, bn)
                signs.append(np.sign(s))
            if site in gated:
                assert all(np.array_equal(signs[0], q) for q in signs), site
                share = float((signs[0] < 0).mean())
                assert 0.125 <= share <= 0.375, (site, share)
    blob = gw.gated_blob(size)
    a, back = pkg.weights.unpack_blob(blob)
    assert a == arch
    for k, v in back.items():
        assert np.array_equal(v, sd[k]), k
        assert np.isfinite(v).all(), k          # (the FOLDED conv weights are the tracer's, normal fp16 numbers: tests/test_tracer_cpu.py)


@pytest.mark.parametrize("size", SIZES)
def test_activity(size):
    st = state(size)
    x = tw.preprocess(st["org"][st["is_imp"]], st["pred"][st["is_imp"]])
    got = gw.site_statistics(st["sd"], x, gw.gated_sites(size))
    print(f"size {size}: share of the light cone the bias clips:", {k: f"{v[1]:.2f}" for k, v in got.items()})
    for site, (_, share) in got.items():
        assert 0.2 <= share <= 0.8, (site, share)


@pytest.mark.parametrize("size", SIZES)
def test_cap_on_empty_comparisons(size):
    st = state(size)
    empty = float((st["ref"] == 0.0).mean())
    print(f"size {size}: {empty:.2%} of the (CU, logit) pairs have a float64 expectation of exactly 0 ({st['is_zero'].mean():.2%} are the zero CUs)")
    assert empty <= 0.05
    assert (st["ref"] >= 0).all() and (st["ref"] <= st["M"]).all(), "gates only take away: 0 <= forward64 <= M"


@pytest.mark.parametrize("size", SIZES)
def test_tolerance(size):
    t0 = time.time()
    err = gw.emulated_errors(size)
    fast, exact = 8 * err["fp16"], np.maximum(8 * err["hilo"], 8 * gw.GATED_ORACLE_MEASURED[size])
    print(f"size {size}: rho_fast {[f'{v:.3e}' for v in fast]} rho_exact {[f'{v:.3e}' for v in exact]} (8 x hilo emulation {[f'{8 * v:.3e}' for v in err['hilo']]}) {time.time() - t0:.1f} s")
    for name, got, table in (("RHO_GATED_FAST", fast, gw.RHO_GATED_FAST), ("RHO_GATED_EXACT", exact, gw.RHO_GATED_EXACT)):
        want = np.asarray(table[size])
        assert want.shape == got.shape and (np.abs(want - got) <= 0.02 * got).all(), f"gw.{name}[{size}] = {want.tolist()} is not what the emulation gives: {got.tolist()}"
    assert (np.asarray(gw.RHO_GATED_EXACT[size]) >= 8 * gw.GATED_ORACLE_MEASURED[size]).all()
    # (no order between the two tables is asserted: in the ungated deep stages of 32 and 64 an impulse's activations are fp16 subnormals, where the lo half is
    # 0 and the pair rounds as a single fp16 does; the two emulations' largest errors there differ by which roundings happen to cancel -- 32, last head:
    # 6.0e-4 (hilo) against 2.8e-4 (fp16))
    assert (np.asarray(gw.RHO_GATED_FAST[size]) <= np.asarray(tw.RHO_FAST[size])).all(), "less flows than under the tracer weights: the gated rho is no larger"


@pytest.mark.parametrize("size", SIZES)
def test_power(size):
    st = state(size)
    muts = gw.mutations(size)
    n_places = len(gw.places(size))
    assert n_places == {128: 9, 64: 8, 32: 6, 16: 3}[size] and len(muts) == 2 * n_places + sum(p[0].endswith(".out") for p in gw.places(size))
    last = gw.gated_sites(size)[-1]
    assert any(m[0] == "norelu" and m[1] == last for _, m in muts)
    tables = [("rho_fast", gw.rho(size, False))] + ([("rho_exact", gw.rho(size, True))] if size in EXACT_BY_DEFAULT else [])
    missed = []
    t0 = time.time()
    for name, mut in muts:
        idx = gw.mutation_cus(size, mut, st["labels"], st["org"], st["is_zero"], st["is_imp"])
        got = gw.reference(size, st["org"][idx], st["pred"][idx], mutation=mut, sd=st["sd"])
        move = np.abs(got - st["ref"][idx])
        M = st["M"][idx]
        line = []
        for tname, rho in tables:
            ratio = np.where(M > 0, move / np.where(M > 0, rho[None, :] * M, 1.0), 0.0)
            i, k = np.unravel_index(np.argmax(ratio), ratio.shape)
            line.append(f"{ratio.max():.1f} x {tname} at {st['labels'][idx[i]]} logit {k}")
            listed = tname == "rho_fast" and (mut[0], mut[1]) in gw.UNSEEN[size]
            if (ratio.max() > 2) == listed:
                missed.append(((mut[0], mut[1]), tname, round(float(ratio.max()), 2)))
        zero_moved = bool((got[0] != 0.0).any())
        print(f"size {size}: {name}: {'; '.join(line)}; zero CU {'moved to ' + str(got[0][got[0] != 0][:1].tolist()) if zero_moved else 'stays 0.0'}")
        if mut[0] == "norelu" and mut[1] == last:
            # (16 x 16: the last gated site is layer0.1.out, which no head pools; the ungated stages behind it clip the negative pixel again)
            assert zero_moved == (size != 16), name
    print(f"size {size}: {len(muts)} mutations {time.time() - t0:.1f} s")
    assert all(gw.seen_mutations(size).count(nm) == 1 for nm in muts if (nm[1][0], nm[1][1]) not in gw.UNSEEN[size])
    assert {m[0] for _, m in gw.seen_mutations(size)} == set(gw.KINDS), "no kind may be dropped"
    assert not missed, f"gw.UNSEEN[{size}] is not what is measured -- pairs on the wrong side of 2 x rho x M: {missed}"


@pytest.mark.parametrize("size", SIZES)
def test_agrees_with_the_c_oracle_and_the_torch_port(pkg, size):
    from oracle import Oracle
    from oracle.torch_port import TorchPort
    st = state(size)
    pos = tw.sample_positions(size, 6, 8)            # 4 corners + 6 border + 8 interior = 18 positions x 2 planes, and 8 dense CUs
    cases = [tw.impulses(size, plane, pos) for plane in (0, 1)] + [pkg.synth.make_patches_bulk(size, 8, 31)]
    org, pred = (np.concatenate([c[i] for c in cases]) for i in (0, 1))
    n = len(org)
    assert n == 44
    want = gw.reference(size, org, pred, sd=st["sd"])
    M = gw.magnitude(size, org, pred)
    z = np.zeros(n, np.int32)
    blob = gw.gated_blob(size)
    worst = {}
    for name, fwd in (("C oracle", lambda: Oracle(blob).forward(org, pred, z, z, threads=8)[0]), ("torch port", lambda: TorchPort(blob).forward(org, pred, z, z, threads=8)[0])):
        got = fwd().astype(np.float64)
        rel = np.abs(got - want) / M
        worst[name] = float(rel.max())
        print(f"size {size}: forward64 vs {name}, {n} CUs: max |difference| / M {rel.max():.2e} (impulses {rel[:36].max():.2e}, dense {rel[36:].max():.2e})")
        assert rel.max() <= ORACLE_BOUND, name
    assert worst["C oracle"] <= gw.GATED_ORACLE_MEASURED[size], "gw.GATED_ORACLE_MEASURED (the floor under RHO_GATED_EXACT) is no longer what is measured"
    assert worst["torch port"] <= 4 * gw.GATED_ORACLE_MEASURED[size]
