"""No-GPU checks of fp16 / bf16 feature maps (gwbp_scatter_typed and friends): the C ABI, the assembly gate of the new
256-channel object, and the promise that the fp32 kernels compile to exactly the code they had before the half-map
instantiations were split off into their own translation units."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import pytest

from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-munsafe-fp-atomics", "-fvisibility=hidden", "-Wno-inline-asm", "-S", "--cuda-device-only"]
TYPED = ("gwbp_scatter_typed", "gwbp_scatter_upsampled_typed", "gwbp_scatter_bilinear_typed", "gwbp_scatter_tokens_typed")

# sha256[:16] of every device function body (instructions, labels normalised) of the fp32 objects, compiled from the sources
# as they were before the kernel bodies moved into scatter_wide_kernel.h / scatter_full_kernel.h / token_kernel.h
PARENT_BODIES = {
    ("scatter_wide", "-O3"): ["06f9c65def698c5a", "8f2028aae87c57c9"],
    ("scatter_wide", "-O2"): ["0c74f0b0172f6399", "6093013d3551116a"],
    ("scatter_full", "-O3"): ["23051e294b3bf7cd", "672f05b2dddf4e66", "8a1926ac5f0e2736", "b596273e8631cf03", "b9499e580c851fc1"],
    ("scatter_full", "-O2"): ["55115ace76f16b95", "a94cc26409e8ba02", "b596273e8631cf03", "b9499e580c851fc1", "c8d440eea9a81357"],
    ("token", "-O3"): ["32a63de275f8e5de", "47a7c22a9c87a449", "5f3713f026c98507", "93134edbe9e47385", "9aa91f39a35f5651",
                       "a5a016a5bea15d59", "bfe3afbe423a279b", "f466a74e4df33e82", "fcda1a48108fb9ce"],
    ("token", "-O2"): ["25f3f53117d8cff9", "32a63de275f8e5de", "4314316a79aeb313", "47a7c22a9c87a449", "6b595cb785dfb158",
                       "8fd2b44516b6ede9", "9aa91f39a35f5651", "c85700cd8ebd9fc2", "f466a74e4df33e82"],
}


def _bodies(path):
    """{symbol: [instruction lines]} of the functions in a hipcc -S file; comments, directives and the names of local branch
    labels are dropped (a label's position stays, as "L:"), so that a renamed template instance with the same code hashes the
    same."""
    out, name, cur = {}, None, None
    for raw in open(path):
        s = raw.strip()
        m = re.match(r"^(_Z\S+):", s)
        if m:
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            out[name], name = cur, None
            continue
        if s.startswith(".LBB"):
            cur.append("L:")
            continue
        s = s.split(";")[0].strip()
        if s and not s.startswith("."):
            cur.append(re.sub(r"\.LBB\d+_\d+", "LBB", s))
    return out


def _digest(path):
    return sorted(hashlib.sha256("\n".join(b).encode()).hexdigest()[:16] for b in _bodies(path).values())


def _compile(tmp_path, name, opt):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / f"{name}{opt}.s"
    subprocess.check_call([HIPCC, opt, *FLAGS, "-o", str(out), os.path.join(_lib.CSRC, f"{name}.hip")], stderr=subprocess.DEVNULL)
    return str(out)


def test_map_types_and_typed_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    for name, val in (("GWBP_MAP_F32", 0), ("GWBP_MAP_F16", 1), ("GWBP_MAP_BF16", 2)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in TYPED:
        assert f"GWBP_API int {fn}(" in hdr, fn
        assert fn in exported and fn in _lib.EXPORTS, fn


def test_header_with_map_types_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gwbp.h"\nint main(void) { return GWBP_MAP_BF16 == 2 ? 0 : (int)sizeof(&gwbp_scatter_typed); }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("fn", TYPED)
@pytest.mark.parametrize("code", [-1, 3, 7])
def test_unknown_map_type_is_einval_before_any_device_call(fn, code):
    """An unknown type code is refused before the caps, the workspace or the view are looked at (all NULL here): no device
    call can have happened."""
    L = _lib.lib()
    f = getattr(L, fn)
    n = len(_lib.ARGTYPES[fn])
    args = [None] * n
    args[5] = code  # caps, workspace, bytes, view, feats, map_type
    for i, t in enumerate(_lib.ARGTYPES[fn]):
        if args[i] is None and t in (C.c_int64, C.c_int32, C.c_size_t):
            args[i] = 0
        elif args[i] is None and t is C.c_float:
            args[i] = 1.0
    assert f(*args) == -1  # GWBP_EINVAL
    assert b"unknown map type" in L.gwbp_last_error_string()


# argument index -> the value that fails the function's one check of its index maps (NULL caps: refused before any device call)
UPSAMPLED_BAD = [{10: None}, {11: None}]                                     # ymap, xmap
BILINEAR_BAD = [{10: 0}, {11: 0}, {12: None}, {13: None}, {14: None}, {15: None}]  # lr_h, lr_w, y0, ly, x0, lx


@pytest.mark.parametrize("fn, bad, msg", [("gwbp_scatter_upsampled_typed", b, "needs both index maps") for b in UPSAMPLED_BAD] +
                         [("gwbp_scatter_bilinear_typed", b, "needs both index maps, both weight maps and the map size")
                          for b in BILINEAR_BAD])
@pytest.mark.parametrize("map_type", [_lib.MAP_F32, _lib.MAP_F16, _lib.MAP_BF16])
def test_typed_index_map_checks_name_their_function(fn, bad, msg, map_type):
    """A missing index or weight map is refused before the caps are looked at, in the name of the function that runs the check:
    GWBP_MAP_F32 is the untyped function's call, so the message is that function's."""
    L = _lib.lib()
    buf = (C.c_char * 64)()
    fake = C.c_void_p(C.addressof(buf))
    args = [None, None, 0, None]
    for i, t in enumerate(_lib.ARGTYPES[fn][4:], 4):
        args.append(bad[i] if i in bad else map_type if i == 5 else 4 if t in (C.c_int64, C.c_int32) else 1.0 if t is C.c_float
                    else fake)
    assert getattr(L, fn)(*args) == -1
    name = fn[:-len("_typed")] if map_type == _lib.MAP_F32 else fn
    assert L.gwbp_last_error_string() == f"{name} {msg}".encode()
    for i, v in bad.items():  # and with the argument mended the call reaches the caps
        args[i] = 4 if v == 0 else fake
    assert getattr(L, fn)(*args) == -1 and L.gwbp_last_error_string() == b"null caps"


@pytest.mark.parametrize("opt", ["-O3", "-O2"])
def test_half_wide_object_passes_the_assembly_gate(tmp_path, opt):
    """scatter_wide_half.hip: four k_scatter_wide instantiations (fp16, bf16 x full resolution, bilinear) under every check the
    fp32 object gets -- reserved SGPR tuples, in-flight landing registers, next-free SGPR 100, the v_readfirstlane hazard -- and
    within the register budget that leaves one front-stage wave per SIMD beside the kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    s = _compile(tmp_path, "scatter_wide_half", opt)
    assert check_asm_hazards.check_wide(s, kernels=4) == []
    inst = check_asm_hazards.wide_instantiations(s)
    assert sorted(inst) == ["Lb0ELi1E", "Lb0ELi2E", "Lb1ELi1E", "Lb1ELi2E"], inst
    assert all(97 <= v <= 104 for k, v in inst.items() if k.startswith("Lb0E")), inst
    assert all(97 <= v <= 112 for k, v in inst.items() if k.startswith("Lb1E")), inst
    # and the gate is not vacuous: the four-kernel object fails the two-kernel count
    assert any("instantiations" in m for m in check_asm_hazards.check_wide(s))


@pytest.mark.parametrize("opt", ["-O3", "-O2"])
@pytest.mark.parametrize("name", ["scatter_wide", "scatter_full", "token"])
def test_fp32_objects_compile_to_the_code_they_had(tmp_path, name, opt):
    assert _digest(_compile(tmp_path, name, opt)) == PARENT_BODIES[(name, opt)]


def test_half_objects_hold_only_half_instantiations(tmp_path):
    for name, pat in (("scatter_full_half", r"k_scatter_fullILb0ELi[12]ELi([0-9])EE"),
                      ("token_half", r"k_token_applyILi\dELb1ELb[01]ELi([0-9])EE")):
        types = {m.group(1) for b in _bodies(_compile(tmp_path, name, "-O3")) for m in [re.search(pat, b)] if m}
        assert types == {"1", "2"}, (name, types)


def test_cli_map_dtype_parses_and_defaults_to_float32():
    sys.path.insert(0, ROOT)
    import run_backproject
    p = run_backproject.build_parser()
    assert p.parse_args([]).map_dtype == "float32"
    assert p.parse_args(["--map-dtype", "keep"]).map_dtype == "keep"
    with pytest.raises(SystemExit):
        p.parse_args(["--map-dtype", "float16"])
