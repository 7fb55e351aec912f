"""The two forms of the batch link's filter bank agree bit for bit (CPU, no GPU needed).

bl_gsff<GATED = true> is k_batch's: ring entries requested only for full windows, seeding and mode cascade behind one
compare of the history length with a per-lane threshold that stands in for the stored mode.  bl_gsff<GATED = false> is
k_track_lanes's, the form both kernels shared before.  scripts/gsff_host_check.py builds both out of batch_link.h with the
host compiler and runs random tracks through them as their kernels would -- births on lanes that still hold an earlier
track's state, handles of one to three filters, launches that end (threshold -> stored mode -> threshold) at random
frames -- comparing every output, every field of the seat and the ring in every frame."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gated_filter_bank_equals_the_ungated_one_on_the_host():
    spec = importlib.util.spec_from_file_location("gsff_host_check", os.path.join(ROOT, "scripts", "gsff_host_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.compiler() is None:
        pytest.skip("no host C++ compiler")
    status, out = mod.run(trials=1500)
    print(out)
    assert status == 0, out
    assert out.startswith("ok:") and int(out.split()[1]) > 100000
