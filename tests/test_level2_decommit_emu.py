"""Decommitment on device handles (`lmn_tree_decommit`, `lmn_col_gather`) on the TEST-ONLY emulation build: the host walk
that plans an opening, the indexing of the two kernels, the refusals, and a whole proof whose trees keep only handles -
against the oracle's `MerkleTree.decommit` / `verify_decommitment`.  The checks themselves are in
tests/level2_decommit_checks.py; tests/test_gpu_level2_decommit.py runs them on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import level2_decommit_checks as dc
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_lib(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return backend.Library(so)


def test_decommit_symbols_are_exported_and_bound(emu_lib):
    for name in ("lmn_tree_decommit", "lmn_col_gather"):
        assert name in backend.EXPORTS
        getattr(emu_lib.lib, name)
    assert backend.API_VERSION == 6


def test_openings_equal_the_oracle_and_verify(emu_lib):
    dc.check_oracle(emu_lib)


def test_gather_equals_numpy_indexing(emu_lib):
    dc.check_gather(emu_lib)


def test_refusals_name_the_argument_and_leave_context_and_tree_usable(emu_lib):
    dc.check_refusals(emu_lib)


def test_whole_proofs_without_whole_column_downloads(emu_lib):
    dc.check_whole_proof(emu_lib)


def test_batch_library_decommits_like_the_main_one():
    """libluminair_hip_batch.so is built from the same sources: what lmn_col_commit does there, the new calls do too"""
    from oracle.merkle import MerkleTree
    from test_batch_emu import _build
    lib = backend.Library(_build())
    ctx = backend.Context(0, None, lib)
    rng = np.random.default_rng(3)
    host = [rng.integers(0, dc.P, size=s, dtype=np.uint64).astype(np.uint32) for s in ((3, 64), (2, 16))]
    handles = [ctx.col_from_cpu(a) for a in host]
    tree = ctx.commit(handles)
    ref = MerkleTree([c for a in host for c in a])
    q = {6: [0, 9, 10, 63], 4: [2]}
    vals, hw, cw = tree.decommit(handles, q)
    assert tree.root() == ref.root() and (vals.tolist(), hw, cw.tolist()) == ref.decommit(q)
    assert np.array_equal(handles[0].gather([63, 0, 0]), host[0][:, [63, 0, 0]])
    with pytest.raises(backend.LuminairBackendError) as e:
        tree.decommit(handles[:1], q)
    assert e.value.code == backend.ERR_INVALID_ARGUMENT and "cols" in str(e.value)
    tree.free()
    for h in handles:
        h.free()
    ctx.close()
