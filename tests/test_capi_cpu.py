"""No-GPU checks of the C-ABI library: it loads, exports every symbol include/gwbp.h declares, and its pure-host
entry points (workspace sizing, argument validation, error strings) behave.  No compute calls."""
import ctypes as C
import os
import re

import pytest

import gsbp_amd
from gsbp_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gwbp.h")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gwbp_[a-z_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    gsbp_amd.build()
    lib = _lib.lib()
    syms = declared_symbols()
    assert len(syms) >= 13 and set(syms) == set(_lib.EXPORTS)
    for s in syms:
        assert getattr(lib, s) is not None
    assert b"gfx950" in lib.gwbp_version()


def test_library_exports_nothing_but_the_declared_symbols():
    """"no C++ types across it".  The dynamic symbol table of libgwbp.so equals the GWBP_API prototypes of
    include/gwbp.h in BOTH directions: -fvisibility=hidden + csrc/gwbp.map localise the launchers (which take hipStream_t), the
    kernel host stubs and hipcc's __hip_cuid_* markers (round 5 exported 42 mangled gwbp::* symbols beside the 23)."""
    import subprocess
    gsbp_amd.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == declared_symbols(), sorted(set(exported) ^ set(declared_symbols()))


def test_header_is_plain_c():
    """a C ABI -- the header a foreign binding (cgo, JNI, ctypes generators) would include must compile as C99 and
    as C++ on its own, with no torch / HIP include behind it."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HDR])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HDR])
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)  # (the comments may NAME torch and HIP types)
    assert set(re.findall(r"#include\s*<([^>]+)>", code)) == {"stddef.h", "stdint.h"}
    assert not re.search(r"\b(at::|torch|hipStream_t|hipError_t)\b", code)


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.View) == 16 * 4 + 9 * 4 + 2 * 4 + 4 * 4
    assert C.sizeof(_lib.Caps) == 8 * 3 + 4 * 4
    assert C.sizeof(_lib.Stats) == 32


def test_workspace_size_and_argument_validation():
    lib = _lib.lib()
    n = C.c_size_t(0)
    caps = _lib.Caps(1_000_000, 16_000_000, 217_088_000, 1600, 1060)
    assert lib.gwbp_workspace_size(C.byref(caps), C.byref(n)) == 0
    # g2d 32 + rect 8 + touched 4 + depth-sort key/value ping-pong 16 B per Gaussian; tile key/value ping-pong 16 B +
    # header 64 B per intersection; 8 B per weight-store entry; the carry slices of
    # the 256-channel scatter (256 workgroups x 1024 rows x 1 KB)
    expect = 1_000_000 * 60 + 16_000_000 * 80 + 217_088_000 * 8 + 256 * 1024 * 1024
    assert expect < n.value < expect * 1.02
    # unknown flag bits are rejected (bit 3 was the removed GWBP_FLAG_GROUP_SCATTER)
    caps_g = _lib.Caps(1_000_000, 16_000_000, 217_088_000, 1600, 1060, 0, 8)
    assert lib.gwbp_workspace_size(C.byref(caps_g), C.byref(C.c_size_t(0))) == -1
    assert b"unknown caps.flags" in lib.gwbp_last_error_string()
    bad = _lib.Caps(-1, 16, 1 << 20, 64, 64)
    assert lib.gwbp_workspace_size(C.byref(bad), C.byref(n)) == -1
    assert b"caps out of range" in lib.gwbp_last_error_string()
    small = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    # null workspace / too-small workspace are rejected before any HIP call
    assert lib.gwbp_project(C.byref(small), None, C.c_size_t(0), C.byref(view), None, None, None, None, None, None,
                            None, None, None) == -1
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255
    assert lib.gwbp_project(C.byref(small), C.c_void_p(addr), C.c_size_t(1024), C.byref(view), None, None, None, None,
                            None, None, None, None, None) == -2
    assert b"workspace too small" in lib.gwbp_last_error_string()
    assert lib.gwbp_finalize(C.c_int64(-1), 8, None, None, None, None) == -1
    # gwbp_blend_scatter_encoded: a map whose rows span 4 GB or more is rejected before any launch (the kernel's per-lane
    # column offsets are 32-bit: ADVICE r5) -- validation only, the pointers are never dereferenced
    nbytes = C.c_size_t(0)
    assert lib.gwbp_workspace_size(C.byref(small), C.byref(nbytes)) == 0
    fake = C.c_void_p(addr)
    view.width, view.height = 64, 64
    wide_stride = (1 << 32) // 4 // 63 + 16  # 63 pixel strides of this many floats pass 4 GB
    wide_stride -= wide_stride % 4
    rc = lib.gwbp_blend_scatter_encoded(C.byref(small), fake, nbytes, C.byref(view), fake, C.c_int64(64 * wide_stride),
                                        C.c_int64(wide_stride), 64, fake, 16, 1.0, 1.0, fake, None, None, None)
    assert rc == -1 and b"32-bit" in lib.gwbp_last_error_string(), lib.gwbp_last_error_string()


# Every entry point that takes (caps, workspace, workspace_bytes, view_host), with what its own arguments need to pass the
# checks it runs BEFORE it binds the workspace: {argument index: value}; every other pointer is a fake aligned address (never
# dereferenced: these calls return before any device call), every other integer 4, every float 1.  The typed scatters are
# called as GWBP_MAP_F32 (the untyped function's call) and as GWBP_MAP_F16.
_LABEL = {5: _lib.LABEL_I32}
BOUND_CALLS = [(name, {}) for name, at in _lib.ARGTYPES.items() if at[:4] == _lib._WSV and not name.endswith("_typed")
               and name not in ("gwbp_project_camera", "gwbp_scatter_labels", "gwbp_scatter_mask_features", "gwbp_vote_labels",
                                "gwbp_vote_projected")]
BOUND_CALLS += [(name, {5: mt}) for name in _lib.ARGTYPES if name.endswith("_typed") for mt in (_lib.MAP_F32, _lib.MAP_F16)]
BOUND_CALLS += [("gwbp_project_camera", {4: 0, 5: 0}), ("gwbp_scatter_labels", _LABEL), ("gwbp_vote_labels", _LABEL),
                ("gwbp_vote_projected", _LABEL),
                ("gwbp_scatter_mask_features", {5: _lib.LABEL_I32, 11: _lib.MAP_F32, 20: _lib.MASK_SLOT_BYTES << 16})]


def _bound_args(name, own, caps, ws, nbytes, view):
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    args = [caps, fake if ws else None, nbytes, view]
    for i, t in enumerate(_lib.ARGTYPES[name][4:], 4):
        if i in own:
            args.append(own[i])
        elif t in (C.c_int64, C.c_int32, C.c_size_t):
            args.append(4)
        elif t is C.c_float:
            args.append(1.0)
        elif t is C.c_void_p:
            args.append(fake)
        elif t._type_ is C.c_int64:  # gwbp_dump_pairs' n_host
            args.append(C.byref(C.c_int64(0)))
        else:                        # const gwbp_pixel_weights *: no map
            args.append(None)
    return args


@pytest.mark.parametrize("name, own", BOUND_CALLS, ids=[f"{n}-{o.get(5, '')}" for n, o in BOUND_CALLS])
def test_caps_workspace_and_view_are_checked_in_that_order_before_any_device_call(name, own):
    """Valid own arguments, then: NULL caps, a NULL workspace, a workspace that is too small, a NULL view and a view larger than
    the caps.  Each is refused with its own code and message before the next is looked at."""
    L = _lib.lib()
    small = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(small), C.byref(nbytes)) == 0
    view, big = _lib.View(), _lib.View()
    view.width, view.height, big.width, big.height = 64, 64, 65, 64
    view.K[0] = view.K[4] = big.K[0] = big.K[4] = 50.0
    f = getattr(L, name)
    for caps, ws, n, v, rc, msg in ((None, True, nbytes, C.byref(view), -1, b"null caps"),
                                    (C.byref(small), False, nbytes, C.byref(view), -1, b"null workspace"),
                                    (C.byref(small), True, C.c_size_t(1024), C.byref(view), -2, b"workspace too small"),
                                    (C.byref(small), True, nbytes, None, -1, b"null view"),
                                    (C.byref(small), True, nbytes, C.byref(big), -1, b"view 65x64 outside caps 64x64")):
        assert f(*_bound_args(name, own, caps, ws, n, v)) == rc, (msg, L.gwbp_last_error_string())
        assert msg in L.gwbp_last_error_string(), (msg, L.gwbp_last_error_string())


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.Engine(10, 64, 64, device="cpu")
    z = torch.zeros(4, 3)
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.rasterization(z, torch.zeros(4, 4), z, torch.zeros(4), z, torch.eye(4)[None], torch.eye(3)[None], 64, 64)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.dirname(_lib.__file__)
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f)).read()
                assert "oracle" not in txt.replace("CPU oracle", "").replace("the oracle", "").replace(
                    "oracle bit", ""), f


def test_profile_build_is_refused_without_explicit_opt_in(tmp_path, monkeypatch):
    """A library whose gwbp_version() says PROFILE (ablation knobs read from the environment, results may be invalid)
    is only ever loaded through an explicit _lib.use_library(path, allow_profile=True); the environment cannot swap the
    product library at all (GWBP_LIB was a developer knob in the product path)."""
    import subprocess
    src = tmp_path / "fake.c"
    src.write_text('const char *gwbp_version(void) { return "libgwbp gfx950 (PROFILE build)"; }\n'
                   'const char *gwbp_last_error_string(void) { return ""; }\n')
    so = tmp_path / "libfake_profile.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setenv("GWBP_LIB", str(so))          # ignored: the package binds to its own in-tree library
    monkeypatch.setenv("GWBP_ALLOW_PROFILE", "1")
    assert _lib._lib_path == _lib.LIB_PATH
    monkeypatch.setattr(_lib, "_lib_path", _lib.LIB_PATH)
    monkeypatch.setattr(_lib, "_allow_profile", False)
    _lib.use_library(str(so))                          # explicit, but without the PROFILE opt-in: refused
    with pytest.raises(_lib.GwbpError, match="PROFILE"):
        _lib.lib()
    assert _lib._lib is None
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    assert not [f for f in os.listdir(pkg) if "profile" in f], "no PROFILE library may sit in the package directory"


@pytest.mark.parametrize("opt", ["-O3", "-O2"])
def test_inline_asm_contracts_of_the_scatter_kernels(tmp_path, opt):
    """k_scatter_wide issues its visit loop's loads / stores / atomics through inline asm with SGPR bases, keeps its scalar
    entry stream in two FIXED SGPR tuples (s[68:83], s[84:99]) and asm-issued loads in flight ACROSS asm statements.  None of
    that is visible to hipcc, so the assembly is checked instead (tools/check_asm_hazards.py; the SAME gate runs inside the
    Makefile for every build variant of the object):
      * no SGPR base written by v_readfirstlane / v_readlane less than 5 wait states before the VMEM instruction that uses it
        (hipcc's hazard recogniser does not look inside inline asm; the first no-compute ablation build faulted on it);
      * no compiler-emitted instruction names s68..s99 (amdgpu_num_sgpr(76) keeps hipcc inside s0..s67), and the kernel
        descriptor still covers them (.amdhsa_next_free_sgpr 100);
      * no compiler-emitted instruction names the landing register of an asm-issued load between the issuing statement and the
        statement that waits for it (round 5: a PROFILE build resolved a phi with v_mov copies IN FRONT of the wait and F was
        wrong by factors at C2 size while every test on the product library passed);
      * the register ALLOCATION, which decides how many front-stage waves fit beside the kernel on a SIMD and the step time
        with it (scatter_wide.hip, "REGISTER BUDGET": 104 = one 64-register front wave per SIMD is the measured optimum, 120
        shuts the front stage out): 97..104 for the full-resolution instantiation, at most 112 for the bilinear one.
    Checked at the product's -O3 and at -O2 (a different schedule and allocation of the same source)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import check_asm_hazards
    flags = [opt, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only"]
    for name in ("scatter_wide", "scatter_full"):
        out = tmp_path / f"{name}.s"
        subprocess.check_call([hipcc, *flags, "-o", str(out), os.path.join(_lib.CSRC, f"{name}.hip")],
                              stderr=subprocess.DEVNULL)
        assert check_asm_hazards.scan(str(out)) == []
        if name == "scatter_wide":
            assert check_asm_hazards.check_wide(str(out)) == []
            _, found = check_asm_hazards.wide_kernel_facts(str(out))
            assert len(found) == 2 and 97 <= found["0"] <= 104 and 97 <= found["1"] <= 112, found


def test_producer_consumer_kernel_has_no_lane_masked_loops(tmp_path):
    """k_blend<kFusedPC> (round 6): its waves wait on an LDS ring.  The first version put a spin loop inside an `if (lane == 0)`
    and a `break` behind the encode; hipcc's control-flow structuriser turned that into a loop which lane 0 left while lanes
    1..63 went round again -- the kernel hung the device.  The source now keeps every ring loop wave-uniform (conditions from
    v_readfirstlane, the LDS atomic alone under the one-lane branch); this checks the RESULT: in the kernel's assembly the only
    loop whose back edge is controlled by the exec mask (`s_andn2_b64 exec, exec, ...`) is the encoder's staging loop."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import subprocess
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only"]
    out = tmp_path / "blend.s"
    subprocess.check_call([hipcc, *flags, "-o", str(out), os.path.join(_lib.CSRC, "blend.hip")], stderr=subprocess.DEVNULL)
    body, on = [], False
    for line in out.read_text().splitlines():
        if re.match(r"_ZN4gwbp7k_blendILi5ELi\d+E\S*:", line):
            on = True
        elif on and line.startswith(".Lfunc_end"):
            break
        elif on:
            body.append(line)
    assert len(body) > 500, "k_blend<kFusedPC, 12> not found in the assembly"
    masked = [ln.strip() for ln in body if "s_andn2_b64 exec, exec" in ln]
    assert len(masked) <= 1, masked
    assert sum("s_sleep" in ln for ln in body) == 2  # the producers' and the consumers' wait, both bounded (kPcMaxSpins)


def test_the_in_flight_register_check_sees_the_round5_hazard(tmp_path):
    """The checker itself: a compiler-looking copy of a landing register placed between an asm-issued load and its wait must be
    reported, and the same copy behind the wait must not."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import check_asm_hazards
    body = """_ZN4gwbp12_GLOBAL__N_114k_scatter_wideILb0EEEvv: ; @k
\t;;#ASMSTART
\tglobal_load_dword v21, v20, s[4:5]
\t;;#ASMEND
%s
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
%s
.Lfunc_end0:
"""
    bad, good = tmp_path / "bad.s", tmp_path / "good.s"
    bad.write_text(body % ("\tv_mov_b32_e32 v60, v21", ""))
    good.write_text(body % ("\tv_mov_b32_e32 v60, v22", "\tv_mov_b32_e32 v61, v21"))
    assert check_asm_hazards.inflight_register_uses(str(bad)) == ["v_mov_b32_e32 v60, v21"]
    assert check_asm_hazards.inflight_register_uses(str(good)) == []
