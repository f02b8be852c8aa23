"""CPU: record_fetch.hip compiled to gfx950 assembly (no GPU needed): the three kernels that read records back keep their
state in registers — no spilled registers, no scratch — and export_blocks_kernel reads its blocks with 16-byte loads
(one global_load_dwordx4 per quad: 1 KiB contiguous per wave)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vector-indexer_amd", "csrc", "record_fetch.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("fetch_match_kernel", "fetch_resolve_gather_kernel", "export_blocks_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> (body, kernel descriptor, resource-usage comment block) of every instantiation of the three"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "record_fetch.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
    subprocess.check_call([HIPCC, *flags, "--cuda-device-only", "-S", "-o", out, SRC], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_ZN2vi\w*?(?:%s)\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % "|".join(KERNELS), text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        usage = text[m.end():].split("\n_ZN", 1)[0]   # the "; ScratchSize: ..." comments between this function and the next
        found[name] = (body, meta, usage)
    return found


def test_all_three_kernels_are_there(kernels):
    for k in KERNELS:
        assert any(k in name for name in kernels), (k, sorted(kernels))
    assert sum("fetch_resolve_gather_kernel" in n for n in kernels) == 2   # with and without the gather
    assert sum("export_blocks_kernel" in n for n in kernels) == 2          # 16-byte and element-wise row stores


def test_no_spills_and_no_scratch(kernels):
    for name, (body, meta, usage) in kernels.items():
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert re.search(r";\s*ScratchSize:\s*\d+", usage), f"{name}: no resource usage found"
        for what in ("ScratchSize", "SGPRSpill", "VGPRSpill", r"\.sgpr_spill_count", r"\.vgpr_spill_count"):
            for m in re.finditer(r"%s:\s*(\d+)" % what, usage):
                assert int(m.group(1)) == 0, f"{name}: {what} {m.group(1)}"
        assert not re.search(r"^\s*scratch_", body, re.M), f"{name}: scratch instructions"


def test_export_reads_its_blocks_with_16_byte_loads(kernels):
    for name, (body, _, _) in kernels.items():
        if "export_blocks_kernel" in name:
            assert len(re.findall(r"^\s*global_load_dwordx4\b", body, re.M)) >= 1, name
