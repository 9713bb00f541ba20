"""The composition polynomial from half of its evaluation domain, on the oracle alone and on the emulation build (tests/emu:
the same HIP sources compiled for the CPU); the checks are in tests/comp_half_checks.py, the GPU's sizes in
tests/test_gpu_comp_half.py."""
import os
import subprocess

import pytest

import comp_half_checks as ch
import test_sharded_prove as tsp
from luminair_amd import backend


@pytest.fixture(scope="module")
def provers(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    p = ch.Provers(backend.Library(so))
    yield p
    p.close()


def test_oracle_quotients_of_every_component_kind_end_at_coefficient_n():
    """every size's composition polynomial of the oracle has no non-zero coefficient above index N, and the polynomial
    rebuilt from rows [0, N) and row N equals it coefficient for coefficient - for all 17 kinds"""
    kinds = set()
    for _, variant, tabs, luts in ch.kind_graphs():
        kinds |= ch.check_oracle_graph(variant, tabs, luts)
    assert kinds == set(range(17)), sorted(kinds)


def test_oracle_mixed_sizes_fold_and_rebuild():
    """a pie of two and one of three sizes: the fold of the smaller polynomials into the larger one's first half and probe"""
    from luminair_amd import synthetic as syn
    ch.check_oracle_graph(ch.PINNED, syn.config2_graph_faithful(1 << 6, 6), None)
    ch.check_oracle_graph(ch.KAT, syn.config3_mixed(7, 6, 5, 7), None)


@pytest.mark.parametrize("e", [1, 2, 3, 7])
def test_oracle_extension_constants(e):
    ch.check_extension_constants(e)


@pytest.mark.parametrize("case", ch.shared_cases() + ch.emu_size_cases(), ids=lambda c: c[0])
def test_emu_proofs_are_byte_identical(provers, case, monkeypatch):
    ch.check_case(provers, case, monkeypatch)


def test_emu_blowup_4_takes_the_whole_domain(provers, monkeypatch):
    from luminair_amd import synthetic as syn
    ch.check_case(provers, ("add 2^13 at log_blowup 2", ch.KAT, syn.config2_add_only(1 << 13, 12), None, False), monkeypatch,
                  log_blowup=2)


def test_emu_sharded_world_2_takes_the_whole_domain(provers, monkeypatch):
    """two ranks as threads of this process (the transport of tests/test_sharded_prove.py): every rank returns the unsharded
    bytes, with and without the switch, and evaluates the whole domain both times"""
    from luminair_amd import synthetic as syn
    tabs = syn.config2_add_only(1 << 13, 13)
    t = [(k, r, len(r)) for k, r in tabs]
    want = provers.ctx(ch.KAT).prove_tables(t)
    lib = provers.lib

    def rank_fn(rank, group):
        ctx = backend.Context(0, lib.default_config(), lib)
        tsp._thread_shard(ctx, group, rank, 0)
        out = []
        for _ in range(2):          # the switch is flipped between the rounds by the main thread's barrier partner: rank 0
            out.append((ctx.prove_tables(t), ctx.timings()["fft_butterflies"]))
            group.exchange(rank, None)
            if rank == 0:
                os.environ[ch.SWITCH] = "1"
            group.exchange(rank, None)
        return out

    class _Q:
        def __init__(self):
            self.items = []

        def put(self, x):
            self.items.append(x)
    q = _Q()
    monkeypatch.delenv(ch.SWITCH, raising=False)
    try:
        tsp._run_thread_ranks(2, q, rank_fn)
    finally:
        os.environ.pop(ch.SWITCH, None)
    assert len(q.items) == 2
    for _, res in q.items:
        assert isinstance(res, list), res
        (p0, b0), (p1, b1) = res
        assert p0 == want and p1 == want and b0 == b1


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("log_rows", [12, 13])
def test_emu_invalid_traces_are_rejected_on_both_paths(provers, monkeypatch, log_rows, which):
    """a broken constraint still ends in LMN_ERR_CONSTRAINTS with and without the switch: at 2^12 rows (the whole domain on
    both paths) and at 2^13 (the smallest table that takes the half-domain path), for two corruptions at different rows"""
    ch.check_invalid_trace(provers.ctx(ch.KAT), monkeypatch, log_rows, which)
