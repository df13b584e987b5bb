"""The registers of pgx_find_mems_pairs_kernel, from the metadata and the assembly of one device compile of pgx_pairs_kernels.hip (as
tests/test_isa_lint.py compiles it, ~20 s; figures by scripts/pairs_isa_stats.py).  The kernel's time follows the length of a trip's instruction
stream, and scalar values that do not fit the 102 scalar registers of a wave are kept in the lanes of a vector register and fetched back with one
vector instruction each: the main loop of the LCE instances once held 82 such values and fetched 165 of them back per trip (266 v_readlane_b32 /
v_writelane_b32 in the body).  Since the kernel takes PgxPairsArgs and reads its rare arguments where they are used, no instance spills:

  all 14 instances: no vector register spilled, no scratch memory;
  the two LCE instances: at most 128 vector registers (four waves per SIMD), static plus dynamic LDS at the widest packed read (24 words per
  thread) within 40 KiB (four workgroups per CU), and v_readlane_b32 + v_writelane_b32 in the body below the pinned bound.

The bound: the LCE instances have 11 such instructions left (none of them a spill: the lane loops of atomic additions the compiler has
combined per wave); 11 + a slack of 8 = 19, far below a quarter (66) of what the body had with the arguments in registers."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LANE_OPS_BOUND = 19  # v_readlane_b32 + v_writelane_b32 in the body of an LCE instance: what the code has (11) + 8
LDS_LIMIT = 40960    # bytes per workgroup that leave four workgroups per CU
PGX_FM_THREADS = 256


def lce_dynamic_lds(pk_words):
    """the dynamic LDS launch_pairs (pgx_batch.hip) asks for an LCE launch: the packed reads, and per thread a seed entry, a suffix array entry and
    five dwords of common prefixes"""
    return pk_words * PGX_FM_THREADS * 4 + PGX_FM_THREADS * (16 + 4 + 20)


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    import pairs_isa_stats

    out = tmp_path_factory.mktemp("pairs_isa") / "pairs.s"
    src = os.path.join(ROOT, "pangenome-index_amd", "csrc", "pgx_pairs_kernels.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "pangenome-index_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    st = pairs_isa_stats.stats(str(out))
    for name, s in sorted(st.items()):
        print(name[:64], s["meta"], "body", s["body"], "loop", s["loop"])
    return pairs_isa_stats, st


def test_no_instance_spills_vector_registers_or_uses_scratch(stats):
    _, st = stats
    assert len(st) == 14, sorted(st)
    for name, s in st.items():
        assert s["meta"]["vgpr_spill_count"] == 0, (name, s["meta"])
        assert s["meta"]["private_segment_fixed_size"] == 0, (name, s["meta"])


def test_lce_instances_fit_four_waves_and_four_workgroups_and_keep_their_scalars_in_registers(stats):
    mod, st = stats
    lce = {name: s for name, s in st.items() if mod.is_lce(name)}
    assert len(lce) == 2, sorted(lce)
    for name, s in lce.items():
        m = s["meta"]
        assert m["vgpr_count"] <= 128, (name, m)
        assert m["group_segment_fixed_size"] + lce_dynamic_lds(24) <= LDS_LIMIT, (name, m["group_segment_fixed_size"], lce_dynamic_lds(24))
        lane_ops = s["body"]["v_readlane"] + s["body"]["v_writelane"]
        assert lane_ops <= LANE_OPS_BOUND, (name, lane_ops, m["sgpr_spill_count"])
        assert m["sgpr_spill_count"] == 0, (name, m)
