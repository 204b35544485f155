"""The EDT's open-space build on rows with more than 508 obstacle columns (widths 513 .. 1024).  The first EDT of such a
map teaches the context that it is open space; from the second on (after sc_ctx_synchronize) the band kernel's build
with the site search runs.  A row whose band has more obstacle columns than the search holds and that is not settled
after the cascade's 175 steps must take the exact 32-bit fallback, not keep the clamped cascade.  Every call is compared
bit-exact with the oracle."""
import numpy as np
import pytest
import torch

import sea_current_amd as sc

pytestmark = pytest.mark.gpu


def _maps(W, H=256):
    left = np.zeros((H, W), np.uint8)
    left[:, :int(0.6 * W)] = 1                    # dense left 60 %, empty right
    rows = np.zeros((H, W), np.uint8)
    rows[::2, :W - 400] = 1                       # every other row set in columns [:W-400]
    return dict(left60=left, rows_every_other=rows)


@pytest.mark.parametrize("W", [1024, 700, 1000])
@pytest.mark.parametrize("kind", ["left60", "rows_every_other"])
def test_open_space_build_many_sites(oracle, W, kind):
    occ = _maps(W)[kind]
    want = oracle.edt(occ)
    ctx = sc.Context(0)
    try:
        dev = torch.from_numpy(occ).cuda()
        for call in range(2):
            d2 = ctx.edt(dev)
            ctx.synchronize()
            got = d2.cpu().numpy()
            assert np.array_equal(got, want), (call, int((got != want).sum()))
    finally:
        ctx.close()
