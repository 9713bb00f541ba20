"""`lmn_trace_check` on the TEST-ONLY emulation build: the kernels' indexing in both table layouts, the tuple tables, the
host side's validation and report - against the oracle's local constraints and a dict fold of its relation entries.  The
checks themselves are in tests/trace_doctor_checks.py; tests/test_gpu_trace_check.py runs them on the MI355X."""
import os
import subprocess

import pytest

import producer_scenarios as ps
import trace_doctor_checks as tc
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_lib(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return backend.Library(so)


def test_trace_check_is_exported_and_bound(emu_lib):
    assert "lmn_trace_check" in backend.EXPORTS
    getattr(emu_lib.lib, "lmn_trace_check")
    assert backend.API_VERSION == 6 and backend.TRACE_REPORT_MAX == 64
    import luminair_amd
    assert luminair_amd.TraceReport is backend.TraceReport and callable(luminair_amd.check_trace)
    assert callable(luminair_amd.Prover.check)


def test_report_structs_have_the_layout_ctypes_computes():
    """the generated `#[repr(C)]` report structs against the Python binding's, as tests/test_rust_bindings.py does for the
    structs of ABI version 6"""
    import ctypes as C
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(tc.ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text, _, funcs, lay = gen.generate()
    assert "pub fn lmn_trace_check(" in text and "lmn_trace_check" in [f[0] for f in funcs]
    assert open(gen.OUT).read() == text                       # the committed file is what the generator writes
    for name, ct in (("lmn_trace_constraint", backend.LmnTraceConstraint), ("lmn_trace_tuple", backend.LmnTraceTuple),
                     ("lmn_trace_report", backend.LmnTraceReport)):
        assert "pub struct %s {" % name in text
        size, _, fields = lay[name]
        assert size == C.sizeof(ct), (name, size, C.sizeof(ct))
        assert [f for f, _, _ in fields] == [f[0] for f in ct._fields_], name
        for fname, off, fsize in fields:
            d = getattr(ct, fname)
            assert (off, fsize) == (d.offset, d.size), (name, fname)


def test_clean_synthetic_pies_report_ok_prove_and_verify(emu_lib):
    """(the 2^17-row Exp2 LUT of config 4 is proved on the MI355X by this test's GPU twin; here it is checked only)"""
    tc.check_clean_synthetic(emu_lib, skip_prove=("config4_black_scholes_shape",))


# the 32x32 shapes are left to the GPU run (the emulation runs one fibre per GPU thread), as in tests/test_producer_scenarios.py
_CPU_BUILDERS = ps.EXPANSIONS + [f for f in ps.OPS if "32x32" not in f.__name__]


def test_producer_scenarios_report_ok(emu_lib):
    """tables written on the device by DeviceGraph.gen_trace; that the same pies prove and verify is
    tests/test_producer_scenarios.py's own assertion on the same builders and is not repeated here"""
    tc.check_clean_producers(emu_lib, _CPU_BUILDERS, prove=False)


@pytest.mark.parametrize("kind", tc.LOCAL_KINDS, ids=lambda k: tc.COMPONENTS[k].name)
def test_every_slot_both_ways(emu_lib, kind):
    tc.check_slots(emu_lib, [kind])


def test_report_ok_iff_the_proof_is_made_and_accepted(emu_lib):
    tc.check_prover_agreement(emu_lib)


def test_imbalances_equal_the_dict(emu_lib):
    tc.check_imbalances(emu_lib)


def test_noncanonical_words(emu_lib):
    tc.check_noncanonical(emu_lib)


def test_host_rows_device_rows_and_a_finished_sink_agree(emu_lib):
    tc.check_table_forms(emu_lib)


def test_refusals_use_lmn_proves_codes_and_name_the_table(emu_lib):
    tc.check_refusals(emu_lib)


def test_hot_keys_of_the_range_check(emu_lib):
    """(the unchanged 2^16-row pie is left to the GPU twin: one pass of the emulation over it is enough here)"""
    tc.check_hot_keys(emu_lib, clean_too=False)


def test_batch_librarys_solo_path_reports_the_same(emu_lib):
    from test_batch_emu import _build
    tc.check_batch_solo(emu_lib, backend.Library(_build()))


def test_sharded_context_checks_without_a_collective(emu_lib):
    """a shard is set, no collective is ever called, and the report is the unsharded one"""
    from luminair_amd import synthetic as syn
    tabs = [(k, r.copy()) for k, r in syn.chain_graph(50)]
    tabs[1][1][9, 11] += 1
    cfg = emu_lib.default_config()
    ctx = backend.Context(0, cfg, emu_lib)
    calls = []
    ctx.set_shard(0, 2, lambda buf, nbytes, stream: calls.append(nbytes))
    rep = ctx.check_trace(tc.pie(tabs))
    tc.assert_equals_oracle(rep, tc.Ref(tabs), "sharded context")
    assert not rep.ok and calls == []
    ctx.close()


def test_the_tool_prints_the_report(emu_lib, tmp_path, root):
    """tools/check_trace.py <pie> [settings] on a pie file with one cell changed"""
    import sys
    import numpy as np
    from luminair_amd import synthetic as syn
    tabs = [(k, r.copy()) for k, r in syn.simple_example()]
    tabs[1][1][2, 11] += 1
    path = tmp_path / "pie.npz"
    np.savez(path, **{"kind_%d" % k: r for k, r in tabs})
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_trace.py"), str(path), "--variant", "kat", "--library", emu_lib.path],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr[-2000:])
    assert "table 1 (Mul) row 2: constraint slot 1 non-zero" in r.stdout, r.stdout
