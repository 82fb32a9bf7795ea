"""The selector's launcher sets each kernel's LDS attribute once per process (csrc/fsel/launch.hpp, kernels.hpp: lds_attr_once), while
fsel_setup_kernel and fsel_kdtree_kernel are asked for another size from call to call.  An attribute cached from a small first call would
make a later, larger one fail - which only shows in a FRESH process that starts small, the order no other selector test has."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_small_then_large_then_small_frames_in_a_fresh_process_match_the_oracle():
    """tests/tools/fsel_orders.py: one Context, one FeatureSelector, five calls - H = 2 with 4 cloud points, H = 13 with 4096 (information() as
    well: the setup-only path), 16 frames at H = 13 and at H = 2 (the two-launch setup; one and two teams per XCD), H = 2 again.  Every frame:
    n_selected and selected_ids equal to the FP64 oracle's, fvalues rel < 1e-9; information(): Omega 1e-12, Delta 1e-10 (the tolerances of
    test_gpu_parity.py::test_selector_information_and_ids)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "fsel_orders.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "all steps ok" in r.stdout, r.stdout[-4000:]
