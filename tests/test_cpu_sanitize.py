"""Host sanitizer runs (SURVEY §5 "race detection / sanitizers"; VERDICT r02
item 9).  GPU AddressSanitizer is not available for gfx950 on this pool, so
the host C++ that parses untrusted input runs under ASan + UBSan on the CPU:

  csrc/flac.cpp (the FLAC bitstream decoder / encoder that replaces soundfile
  behind utils.load_audio / save_audio, /root/reference/utils.py:36,87):
  every bundled LibriSpeech clip decoded whole, 20 truncations and 240
  seeded corruptions each, and encoder round trips (8/16/24-bit, mono and
  stereo, ragged last blocks) -- tests/sanitize/flac_fuzz.cpp.

The torch.ops.ainp host layer (csrc/torch_ops.cpp) is built with UBSan as
libainp_torch_ubsan.so; test_gpu_sanitize.py runs it on the GPU box.

  csrc/conv_route.h (which 3x3 conv kernel serves which call, and every
  host-only query derived from it): tests/sanitize/conv_route_check.cpp walks
  the routing table, the accepted extremes included, as a stand-alone program.

  csrc/conv_gen_route.h (the same for the GAN's general convolution):
  tests/sanitize/conv_gen_route_check.cpp, likewise.

  csrc/gemm_route.h (the GEMM launchers' split-K cover rule and the tile
  ainp_gemm_bf16nt takes): tests/sanitize/gemm_route_check.cpp, likewise.

  csrc/spain_plan.h (the SPAIN launchers' shape rules, LDS plans and lane
  route): tests/sanitize/spain_plan_check.cpp, likewise."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-audio-inpainting_amd", "csrc")


@pytest.fixture(scope="module")
def sanitize_build():
    r = subprocess.run(["make", "-C", CSRC, "sanitize"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(CSRC, "build", "flac_fuzz")


@pytest.mark.timeout(900)
def test_flac_codec_under_asan_ubsan(sanitize_build):
    clips = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "flac", "*.flac")))
    assert len(clips) == 9
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sanitize_build] + clips, capture_output=True, text=True, timeout=800,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "flac_fuzz OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    assert out.count("mutated decodes") == 9


def test_torch_ops_ubsan_library_built(sanitize_build):
    so = os.path.join(ROOT, "ml-audio-inpainting_amd", "ainp", "libainp_torch_ubsan.so")
    assert os.path.exists(so)
    r = subprocess.run(["readelf", "-d", so], capture_output=True, text=True)
    assert "libubsan" in r.stdout


def test_conv_route_table_under_asan_ubsan(sanitize_build):
    """Every cell of the routing table refuses with a known message or names a
    kernel whose grid / row counts fit what the launchers cast them to and the
    workspace bounds, with no overflow at N = 65535, H = W = 2^24 (2^31 - 1
    for the data gradient); and the model's convs run the kernels DESIGN
    section 4 names."""
    exe = os.path.join(os.path.dirname(sanitize_build), "conv_route_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "conv_route_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    # "model <fp32|bf16> <Cin>-><Cout> fwd=<kernel> dgrad=<kernel> wgrad=<kernel>"
    model = {tuple(line.split()[1:3]): dict(kv.split("=") for kv in line.split()[3:])
             for line in out.splitlines() if line.startswith("model ")}
    assert len(model) == 10
    for prec in ("fp32", "bf16"):
        # row strips for 1 <-> 16 (the data gradient of the 16 -> 1 conv runs 1 -> 16)
        assert model[prec, "1->16"]["fwd"] == "rows_1to16"
        assert model[prec, "16->1"]["fwd"] == "rows_16to1"
        assert model[prec, "16->1"]["dgrad"] == "rows_1to16"
        assert model[prec, "1->16"]["wgrad"] == model[prec, "16->1"]["wgrad"] == "strip_cl"
        # x6q for 32 -> 16, forward and the 16 -> 32 conv's data gradient
        assert model[prec, "32->16"]["fwd"] == "x6q" and model[prec, "16->32"]["dgrad"] == "x6q"
        assert model[prec, "32->16"]["dgrad"] == "x6p"
    # x6p for 16 -> 32 and 32 -> 64
    assert model["fp32", "16->32"]["fwd"] == model["fp32", "32->64"]["fwd"] == "x6p"
    assert model["fp32", "32->64"]["dgrad"] == "x6_tiled"
    assert [model["fp32", p]["wgrad"] for p in ("16->32", "32->64", "32->16")] == \
        ["x6s", "x6", "x6s"]
    # the LDS-DMA kernels under bf16 with bf16 channel-last source and output
    assert model["bf16", "16->32"]["fwd"] == model["bf16", "32->64"]["fwd"] == "fwd_b16dma"
    assert model["bf16", "32->64"]["dgrad"] == "dgrad_b16dma"
    assert model["bf16", "32->64"]["wgrad"] == "wgrad_b16dma"


def test_conv_gen_route_table_under_asan_ubsan(sanitize_build):
    """Every cell of the general convolution's routing table refuses with a
    known message or names a kernel whose grids are positive and within the
    launch limits, whose K splits cover every K tile with none empty, whose
    workspace holds the split-K partial sums and whose statistic rows are its
    pixel tiles; the oversized shape saturates instead of overflowing."""
    exe = os.path.join(os.path.dirname(sanitize_build), "conv_gen_route_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "conv_gen_route_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]


def test_gemm_route_under_asan_ubsan(sanitize_build):
    """splitk_covers equals the launchers' former two-product expression
    wherever that cannot overflow and refuses cleanly at kc = INT64_MAX,
    K = INT64_MAX, nsplit = 65535; route_gemm_bf16nt equals the former launcher
    condition under both AINP_GEMM16_256 settings and names the kernels DESIGN
    section 4 names for the layer-0 GEMMs."""
    exe = os.path.join(os.path.dirname(sanitize_build), "gemm_route_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "gemm_route_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    # "model gemm16_256=<0|1> g256_bk64=<0|1> proj=<kernel> dx=<kernel> dw=<kernel>"
    model = {tuple(line.split()[1:3]): dict(kv.split("=") for kv in line.split()[3:])
             for line in out.splitlines() if line.startswith("model ")}
    assert len(model) == 4
    g16 = "g16::gemm_bf16nt_kernel"
    for key, m in model.items():
        assert m["dx"] == m["dw"] == g16, key
    # the split layer-0 projection on the 256 x 256 tile; AINP_GEMM16_256=0: on g16
    assert model["gemm16_256=1", "g256_bk64=0"]["proj"] == "g256::gemm_bf16nt_256_kernel"
    assert model["gemm16_256=1", "g256_bk64=1"]["proj"] == "g256::gemm_bf16nt_256b_kernel"
    assert model["gemm16_256=0", "g256_bk64=0"]["proj"] == g16
    assert model["gemm16_256=0", "g256_bk64=1"]["proj"] == g16


def test_spain_plan_under_asan_ubsan(sanitize_build):
    """Over every legal (w, red) of the window solvers, every legal M of the
    whole-signal solver and their neighbours outside: the plan's sizes, lgN and
    lane route equal the launchers' former expressions, the shape rules refuse
    what they refused with the former messages, and every LDS plan fits a CU."""
    exe = os.path.join(os.path.dirname(sanitize_build), "spain_plan_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "spain_plan_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
