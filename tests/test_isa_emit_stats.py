"""Static checks on the gfx950 code of k_emit_stats, the launch that holds the bodies of k_rank_emit and k_read_stats (no GPU: hipcc
cross-compiles)."""
import os, shutil, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_the_fused_kernels_long_read_merge_is_the_one_of_k_read_stats():
    """the statistics waves of k_emit_stats merge the slices of a long read as k_read_stats does, fence-free: returning per-bin adds, the
    wait for their values, then the slices-done counter's add (tools/isa_stats.py: check_long_merge, on the fused kernel's text)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools/isa_stats.py"), "--check-long-merge", "k_emit_stats"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "17 returning per-bin adds" in r.stdout
