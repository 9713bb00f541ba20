"""The composition polynomial built from half of its evaluation domain (csrc/phase_composition.cpp; docs/HISTORY.md
"Composition from half of its domain"): the checks shared by tests/test_comp_half_emu.py (emulation build, CPU suite) and
tests/test_gpu_comp_half.py (MI355X).

Two kinds of checks:
  * oracle only - the fact the change rests on (a component's quotient on its 2N-point domain has no coefficient above
    index N) and the identities that rebuild it from rows [0, N) and the one row N, for every component kind;
  * whole proofs - the default path, LMN_COMP_FULL_DOMAIN=1 and the oracle give the same bytes, and `fft_butterflies` of the
    timings says which path a proof took."""
import os

import numpy as np

from luminair_amd import backend, synthetic as syn
from oracle import air
from oracle.channel import ProtocolVariant
from oracle.fft import domain_twiddles, evaluate, interpolate
from oracle.field import P, U64, m_add, m_inv, m_mul, m_sub, q_add
from oracle.proof import to_bincode
from oracle.prover import NumpyKernels, PcsConfig, eval_component_constraints_on_domain, prove as oracle_prove

KAT, PINNED = ProtocolVariant.KAT, ProtocolVariant.PINNED
SWITCH = "LMN_COMP_FULL_DOMAIN"
MIN_LOG = 13     # the smallest largest-table log size the half-domain path accepts (fft_interp_extend_supported(comp_log - 1))


# ------------------------------------------------------------------------------------------------ oracle only
def kind_graphs():
    """(name, variant, tables, luts): small valid pies that together hold every one of the 17 component kinds; the three LUT
    pairs come with their lookup tables"""
    out = [("chain", KAT, syn.chain_graph(5, 1), None),
           ("linear layer + max", KAT, syn.linear_layer(2, 4, 2, True), None),
           ("sqrt + rem", PINNED, syn.sqrt_rem_graph(5, 3), None),
           ("less-than + range check", PINNED, syn.less_than_graph(19, 4), None)]
    for n, r in (("sin", (-7, 7)), ("exp2", (-7, 7)), ("log2", (1, 15))):
        tabs, luts = syn.activation_graph(5, 5, names=(n,), ranges={n: r})
        out.append((n + " pair", PINNED, tabs, luts))
    x = np.arange(5) - 2
    out.append(("contiguous", PINNED, [(air.KIND_INPUTS, syn.inputs_rows(x, 0, 1)),
                                       (air.KIND_CONTIGUOUS, syn.contiguous_rows(x, node=2, input_id=0))], None))
    return out


def half_inverse(vals, e):
    """coefficients of the polynomial with 2^(e-1) coefficients from its evaluations on storage rows [0, 2^(e-1)) of the
    2^e-point domain: the inverse layers 0 .. e-2 on the first half of that domain's tables, scaled by 2^-(e-1)"""
    n = e - 1
    _, itws = domain_twiddles(e)
    a = np.asarray(vals, dtype=U64)
    lead = a.shape[:-1]
    for i in range(n):
        a = a.reshape(lead + (1 << (n - 1 - i), 2, 1 << i))
        v0, v1 = a[..., 0, :], a[..., 1, :]
        t = itws[i][:1 << (n - 1 - i), None]
        a = np.stack([m_add(v0, v1), m_mul(m_sub(v0, v1), t)], axis=-2)
    return m_mul(a.reshape(lead + (1 << n,)), m_inv(pow(2, n, P)))


def rebuild_from_half(first_half, probe, e):
    """(4, N) evaluations on rows [0, N) and the (4,) evaluations at row N -> the (4, 2N) coefficients, by the identities:
    g = half_inverse(first half); c = (g(row N) - p(row N)) / 2w; coefficient 0 -= wc, coefficient N = c"""
    N = 1 << (e - 1)
    w = int(domain_twiddles(e)[0][e - 1][0])
    g = half_inverse(first_half, e)
    g_probe = evaluate(g, e)[:, N]
    c = m_mul(m_sub(g_probe, np.asarray(probe, dtype=U64)), m_inv(2 * w % P))
    out = np.zeros((4, 2 * N), dtype=U64)
    out[:, :N] = g
    out[:, 0] = m_sub(g[:, 0], m_mul(c, w))
    out[:, N] = c
    return out


class _Seen(Exception):
    pass


class HalfDomainKernels(NumpyKernels):
    """NumpyKernels whose `composition` also builds every size's polynomial from half of its domain, compares the two and
    records the kinds and sizes it has seen; it then ends the proof (the rest of it is not what is tested)."""

    def __init__(self):
        self.kinds, self.sizes, self.top_nonzero = set(), [], []

    def composition(self, instances, tree0, tree1, tree2, elems, powers, n_total):
        want = super().composition(instances, tree0, tree1, tree2, elems, powers, n_total)
        sub, k0 = {}, 0
        for ci in instances:
            e = ci.log_size + 1
            cp, nc = air.component_coeffs(ci.comp, ci.flags, powers, n_total, k0)
            k0 += nc
            main_e = np.stack([evaluate(tree1.coeffs[i], e) for i in range(*ci.main_span)])
            inter_e = np.stack([evaluate(tree2.coeffs[i], e) for i in range(*ci.inter_span)])
            pre_e = [evaluate(tree0.coeffs[i], e) for i in ci.pre_idx]
            val = eval_component_constraints_on_domain(ci, main_e, inter_e, elems, cp, e, pre_e)
            sub[e] = q_add(sub[e], val) if e in sub else val
            self.kinds.add(ci.comp.kind)
        cur_full = cur_half = None
        for e in sorted(sub):
            N = 1 << (e - 1)
            vals = np.ascontiguousarray(sub[e].T)                       # (4, 2N)
            folded = vals if cur_full is None else m_add(vals, evaluate(cur_full, e))
            cur_full = interpolate(folded)
            # the fact: nothing above index N
            self.top_nonzero.append(int(np.count_nonzero(cur_full[:, N + 1:])))
            first, probe = vals[:, :N], vals[:, N]
            if cur_half is not None:
                ext = evaluate(cur_half, e)
                first, probe = m_add(first, ext[:, :N]), m_add(probe, ext[:, N])
            cur_half = rebuild_from_half(first, probe, e)
            assert np.array_equal(cur_half, cur_full), "size 2^%d: rebuilt coefficients differ" % e
            self.sizes.append(e)
        assert all(np.array_equal(cur_half[k], want[k]) for k in range(4))
        raise _Seen()


def check_oracle_graph(variant, tabs, luts):
    K = HalfDomainKernels()
    try:
        oracle_prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=variant, kernels=K, luts=luts)
    except _Seen:
        pass
    assert K.sizes and all(n == 0 for n in K.top_nonzero), (K.sizes, K.top_nonzero)
    return K.kinds


def check_extension_constants(e):
    """LDE(p) = LDE(g) + c * kappa_h on quarter h of the 4N-point domain, kappa_h = (-1)^h w'[h >> 1] - w with w the top
    twiddle of the 2N-point domain and w' layer e-1 of the 4N-point one: the constants k_comp_half_fix adds"""
    rng = np.random.default_rng(e)
    N = 1 << (e - 1)
    p = np.zeros(2 * N, dtype=U64)
    p[:N + 1] = rng.integers(0, P, N + 1, dtype=np.uint64)
    c = int(p[N])
    w = int(domain_twiddles(e)[0][e - 1][0])
    g = p[:N].copy()
    g[0] = (int(g[0]) + w * c) % P
    assert np.array_equal(half_inverse(evaluate(p, e)[:N], e), g)
    lde_p, lde_g = evaluate(p, e + 1), evaluate(g, e + 1)
    w_ext = domain_twiddles(e + 1)[0][e - 1]
    for h in range(4):
        kappa = ((-1) ** (h & 1) * int(w_ext[h >> 1]) - w) % P
        assert np.array_equal(lde_p[h * N:(h + 1) * N], m_add(lde_g[h * N:(h + 1) * N], c * kappa % P)), h
    # the probe is needed: from three layers on, g's value at row N is not its value at row 0
    if e >= 3:
        assert evaluate(g, e)[N] != evaluate(g, e)[0]


# ------------------------------------------------------------------------------------------------ whole proofs
def _sin_pair(n, seed):
    return syn.activation_graph(n, seed, names=("sin",), ranges={"sin": (-7, 7)})


def shared_cases():
    """(id, variant, tables, luts, takes the half-domain path): run on the emulation build and on the GPU"""
    sin_tabs, sin_luts = _sin_pair(5000, 21)
    return [("add 2^13 (smallest accepted)", KAT, syn.config2_add_only(1 << MIN_LOG, 5), None, True),
            ("add 2^12 + inputs 2^13 (two sizes)", PINNED, syn.config2_graph_faithful(1 << 12, 6), None, True),
            ("config3 mixed 13, 12, 11 (three sizes)", KAT, syn.config3_mixed(13, 12, 11, 7), None, True),
            ("sin + sin lookup + inputs (preprocessed columns, second element set)", PINNED, sin_tabs, sin_luts, True)]


def emu_size_cases():
    return [("add 2^12 (below the range: the whole domain)", KAT, syn.config2_add_only(1 << 12, 8), None, False)]


def gpu_size_cases():
    """trace 2^17: the generic four-quarter kernel; 2^18: the first fixed-shape one (RB 6)"""
    return [("add 2^17 (generic strided kernel)", KAT, syn.config2_add_only(1 << 17, 9), None, True),
            ("add 2^18 (fixed-shape strided kernel)", KAT, syn.config2_add_only(1 << 18, 10), None, True)]


class Provers:
    """one context per protocol variant (and PcsConfig) on a given library"""

    def __init__(self, lib):
        self.lib, self.ctxs = lib, {}

    def ctx(self, variant, log_blowup=1):
        key = (int(variant), log_blowup)
        if key not in self.ctxs:
            cfg = self.lib.default_config()
            cfg.protocol_variant = backend.VARIANT_PINNED if variant == PINNED else backend.VARIANT_KAT
            cfg.log_blowup = log_blowup
            self.ctxs[key] = backend.Context(0, cfg, self.lib)
        return self.ctxs[key]

    def close(self):
        self.ctxs.clear()


def prove_both(ctx, tabs, luts, monkeypatch):
    """(bytes, fft_butterflies) of the default path and of LMN_COMP_FULL_DOMAIN=1"""
    t = [(k, r, len(r)) for k, r in tabs]
    monkeypatch.delenv(SWITCH, raising=False)
    new = ctx.prove_tables(t, luts)
    bf_new = ctx.timings()["fft_butterflies"]
    monkeypatch.setenv(SWITCH, "1")
    full = ctx.prove_tables(t, luts)
    bf_full = ctx.timings()["fft_butterflies"]
    monkeypatch.delenv(SWITCH, raising=False)
    return new, bf_new, full, bf_full


def check_case(provers, case, monkeypatch, kernels=None, log_blowup=1):
    name, variant, tabs, luts, takes_half = case
    new, bf_new, full, bf_full = prove_both(provers.ctx(variant, log_blowup), tabs, luts, monkeypatch)
    want = to_bincode(oracle_prove([(k, r.astype(np.uint64)) for k, r in tabs], PcsConfig(log_blowup=log_blowup),
                                   variant=variant, kernels=kernels, luts=luts))
    assert full == want, name + ": the whole-domain path differs from the oracle"
    assert new == want, name + ": the half-domain path differs from the oracle"
    if takes_half:
        assert bf_new < bf_full, (name, bf_new, bf_full)
    else:
        assert bf_new == bf_full, (name, bf_new, bf_full)


def corrupted_add_tables(log_rows):
    """two corruptions of an Add table that break constraints at different rows (different violated evaluations)"""
    good = syn.config2_add_only(1 << log_rows, 31)[0][1]
    a, b = good.copy(), good.copy()
    a[3, 11] ^= 1                                      # out of row 3
    b[(1 << log_rows) - 5, 9] = (int(b[(1 << log_rows) - 5, 9]) + 1) % P       # lhs of a late row
    return [a, b]


def check_invalid_trace(ctx, monkeypatch, log_rows, which):
    bad = corrupted_add_tables(log_rows)[which]
    for full in (False, True):
        if full:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        try:
            ctx.prove_tables([(0, bad, len(bad))])
        except backend.LuminairBackendError as e:
            assert e.code == backend.ERR_CONSTRAINTS, (log_rows, full, e.code)
        else:
            raise AssertionError("a broken trace was proved (2^%d rows, full domain %s)" % (log_rows, full))
    monkeypatch.delenv(SWITCH, raising=False)
