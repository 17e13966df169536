"""What the cb_ble* entries refuse AFTER they have found a device (tests/test_ble_layout_cpu.py has what comes before): code and
text of each, at S = 3, T = 4, R = 2, n = 2, L = 5.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ble_layout_cpu import CB_EINVAL, _call  # noqa: E402

pytestmark = pytest.mark.gpu


def test_refusals_behind_the_device_check_keep_code_and_text():
    from cherryml_amd.phylogeny_estimation import BleBank
    cx = np.array([[0, 1, 2, -1, 2], [2, 2, -1, 0, 1]], np.int8)
    bad = cx.copy()
    bad[1, 4] = 3
    seqs = np.array([[0, 1, 2, -1, 2], [2, 2, -1, 0, 1], [1, 1, 1, 1, 1], [0, 0, 2, 2, 3]], np.int8)
    with BleBank(np.zeros((4, 2, 3, 3)), np.ones(4), np.ones(2)) as resident:
        handle = resident._h.value
        for side in ("cx", "cy"):
            for entry in ("cb_ble", "cb_ble_batch", "cb_ble_branch_lengths", "cb_ble_site_rates", "cb_site_rate_gather"):
                assert _call(entry, **{side: bad}) == (CB_EINVAL, "ble: state code out of range"), (entry, side)
            assert _call("cb_ble_bank_run", handle=handle, **{side: bad}) == (CB_EINVAL, "cb_ble_bank_run: state code out of range")
        for entry in ("cb_ble", "cb_ble_batch"):
            assert _call(entry, seqs=seqs) == (CB_EINVAL, "cb_ble: state code out of range"), entry
        assert _call("cb_ble_bank_run", handle=handle, seqs=seqs) == (CB_EINVAL, "cb_ble_bank_run: state code out of range")
        assert _call("cb_ble_bank_run", handle=handle, cx=cx)[0] == 0         # the handle is as good as before
    for s2r in ([0, 1, 2, 0, 0], [0, 0, 0, 0, -1]):
        assert _call("cb_ble_branch_lengths", s2r=s2r) == (CB_EINVAL, "cb_ble_branch_lengths: rate index out of range")
    for li in ([0, 4], [-1, 3]):
        assert _call("cb_ble_site_rates", li=li) == (CB_EINVAL, "cb_ble_site_rates: length index out of range")
    assert _call("cb_site_rate_gather", cx=cx) == (CB_EINVAL, "cb_site_rate_gather: negative state code (map gaps to a state)")
    assert _call("cb_site_rate_gather", cy=cx) == (CB_EINVAL, "cb_site_rate_gather: negative state code (map gaps to a state)")
    # and, behind the same check: the sequence count of cb_ble, a device that is not there
    assert _call("cb_ble", n_seqs=0) == (CB_EINVAL, "cb_ble: bad sizes")
    for entry in ("cb_ble", "cb_ble_batch", "cb_ble_branch_lengths", "cb_ble_site_rates", "cb_site_rate_gather"):
        assert _call(entry, device=4096) == (CB_EINVAL, "ble: device 4096 out of range"), entry
    assert _call("cb_ble_bank_create", device=-1) == (CB_EINVAL, "cb_ble_bank_create: device -1 out of range")
