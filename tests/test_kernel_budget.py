"""The register / scratch / LDS budget of the passes that run beside the NIF kernel (DESIGN.md sections 4.1, 4.2, 4.3): the
sharing, memo and accumulate kernels are compiled for gfx950 from their headers alone (no GPU; a few seconds) and the
compiler's resource remarks are held against 80 allocated VGPRs, no scratch and 3 KiB of LDS by
scripts/kernel_resources.py --step-budget --small.  The whole list, trace kernel instances included, is the same script
without --small (more than a minute: the whole library)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_small_step_kernels_fit_beside_two_nif_waves():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "--step-budget", "--small"],
                         capture_output=True, text=True, timeout=300)
    print(run.stdout)
    print(run.stderr[-2000:])
    assert run.returncode == 0, "a kernel is over the budget of 80 allocated VGPRs / no scratch / 3 KiB of LDS"
    rows = {l.split()[0]: l for l in run.stdout.splitlines() if " allocated " in l}
    for k in ("accumulate_kernel", "accumulate4_kernel", "share_claim_kernel", "share_resolve_kernel", "share_expand_kernel",
              "memo_lookup_kernel", "memo_resolve_kernel", "memo_expand_kernel"):
        assert k in rows and rows[k].endswith("ok"), rows.get(k)
    # the one pass that fits beside a NIF pair AND a trace wave (432 + 64 + 16 = 512) stays at one granule pair
    assert " allocated  16 " in rows["share_expand_kernel"], rows["share_expand_kernel"]
