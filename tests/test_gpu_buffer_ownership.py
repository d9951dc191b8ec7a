"""Device memory comes back: a call's temporary buffers when the call returns, a context's buffers
when it is destroyed.  tests/buffer_ownership_probe.py measures free device memory (hipMemGetInfo
through torch.cuda.mem_get_info) in a process of its own, once for both tests; the thresholds leave
256 MiB for what other users of the card may take meanwhile."""
import json
import os
import subprocess
import sys

import pytest

MIB = 1 << 20
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "buffer_ownership_probe.py")


@pytest.fixture(scope="module")
def measured():
    r = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_square_neighborhoods_frees_its_temporaries(measured):
    """682 frames of the default 128 x 128 grid are 682 * 128^2 * 24 B = 255.75 MiB of output, one
    local device buffer per call.  Six calls after a warm-up call: had each kept its buffer, free
    memory would be 1.5 GiB lower; freed at scope exit, they take nothing."""
    m = measured["temporaries"]
    assert (m["size"], m["P"]) == (128, 682) and m["shape"] == [682, 128 * 128, 3]
    drop = m["before"] - m["after"]
    print(f"free before {m['before'] / MIB:.1f} MiB, after six calls {m['after'] / MIB:.1f} MiB, drop {drop / MIB:.1f} MiB")
    assert drop < 256 * MIB


@pytest.mark.gpu
def test_context_destroy_frees_its_buffers(measured):
    """create -> set_g12 -> upload -> run -> close on make_frame_pair(400, seed=2) with pixelsRay = 16:
    free memory after ten, and after a hundred, such cycles is where the warm-up cycle left it.

    What a context that freed nothing would keep: the circle of pixelsRay = 16 has 797 offsets,
    padded to 832 entries, and 400 queries fill ceil(400 / 15) = 27 workgroups of 15 slots
    (lm_groups), so the LM slabs alone (36 B per entry) are 36 B * 832 * 15 * 27 =
    11.6 MiB per context, beside its pyramids, descriptor rows, the matcher's lists and the
    records.  Ten unfreed contexts are then 116 MiB of slabs, which alone would not reach the
    256 MiB threshold; a hundred are 1.13 GiB of slabs, four and a half times it, so it is the
    hundred-cycle reading that a destroy path which frees nothing cannot pass.  Measured with a
    build whose fm3d_ctx_destroy does not delete the context: 378 MiB lower after ten cycles,
    1830 MiB after a hundred (0 MiB and 0 to 2 MiB with one that does)."""
    m = measured["contexts"]
    assert m["kept"][0] > 0 and m["kept"] == [m["kept"][0]] * 101
    for n in ("10", "100"):
        drop = m["before"] - m["after"][n]
        print(f"free before {m['before'] / MIB:.1f} MiB, after {n} contexts {m['after'][n] / MIB:.1f} MiB, drop {drop / MIB:.1f} MiB")
        assert drop < 256 * MIB
