"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950 without a GPU, loads, and exports every
function that include/*.h declares; the Python binding lists the same symbols; and the product refuses to run without
a GPU instead of falling back to anything (no compute calls are made here)."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = re.compile(r"^(?:int|size_t|const char\s*\*)\s*(sgr_\w+)\s*\(", re.M)


@pytest.fixture(scope="module")
def lib():
    from street_gaussians_amd import _native, build
    build.build()  # hipcc cross-compiles for gfx950; a no-op when the objects are up to date
    return C.CDLL(_native.LIB_PATH)


def _declared():
    names = {}
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        for n in DECL.findall(open(h).read()):
            names[n] = os.path.basename(h)
    return names


PROTO = re.compile(r"^(int|size_t|const char\s*\*)\s*(sgr_\w+)\s*\(([^)]*)\)", re.M)
C_KINDS = {"int": "int", "int32_t": "int", "uint32_t": "int", "int64_t": "int64", "size_t": "size_t", "float": "float",
           "double": "double"}
C_RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}


def _c_kind(param):
    """pointer (arrays such as `int64_t counts[6]` included), callback (sgr_alloc_fn) or the scalar's kind"""
    if param.split()[0] == "sgr_alloc_fn":
        return "callback"
    if "*" in param or "[" in param:
        return "pointer"
    return C_KINDS[" ".join(param.split()[:-1])]  # the type without the parameter's name


def _prototypes():
    """name -> (return type, parameter kinds) of every function include/*.h declares"""
    protos = {}
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(h).read(), flags=re.S)
        for ret, name, params in PROTO.findall(text):
            params = [p for p in params.split(",") if p.strip() not in ("", "void")]
            protos[name] = (" ".join(ret.replace("*", "* ").split()), [_c_kind(p) for p in params])
    return protos


def _py_kind(t):
    from street_gaussians_amd._native import ALLOC_FN
    if t is ALLOC_FN:
        return "callback"
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int: "int", C.c_uint32: "int", C.c_int64: "int64", C.c_size_t: "size_t", C.c_float: "float",
            C.c_double: "double"}[t]


def test_library_exports_every_declared_entry_point(lib):
    declared = _declared()
    assert {"sgr_forward", "sgr_backward", "sgr_mark_visible", "sgr_visible_filter", "sgr_knn", "sgr_last_error",
            "sgr_scene_compose_forward", "sgr_ssim_forward", "sgr_sh_grad_from_views"} <= set(declared)
    missing = [f"{n} ({h})" for n, h in declared.items() if not hasattr(lib, n)]
    assert not missing, missing


def test_python_binding_and_headers_agree(lib):
    from street_gaussians_amd import _native
    declared = set(_declared())
    unknown = [n for n in _native.SYMBOLS if n not in declared]
    assert not unknown, f"bound but not declared in include/*.h: {unknown}"
    for n in _native.SYMBOLS:
        assert hasattr(lib, n), n
    # the binding's table and the prototypes agree: return type, parameter count and the kind of every parameter
    protos = _prototypes()
    for n, (restype, argtypes) in _native.SIGNATURES.items():
        ret, kinds = protos[n]
        assert restype is C_RESTYPES[ret], (n, ret)
        assert [_py_kind(t) for t in argtypes] == kinds, n


def test_headers_cite_the_reference_interfaces():
    text = open(os.path.join(ROOT, "include", "sgr.h")).read()
    for ref in ("rasterizer.h", "rasterizer_impl.cu", "simple_knn"):
        assert ref in text
    assert "street_gaussian_model.py" in open(os.path.join(ROOT, "include", "sgr_scene.h")).read()
    assert "loss_utils.py" in open(os.path.join(ROOT, "include", "sgr_loss.h")).read()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour on a machine without a GPU")
def test_product_has_no_cpu_fallback():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from street_gaussians_amd import losses, scene
    from street_gaussians_amd._native import SgrError
    from simple_knn._C import distCUDA2
    st = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False)
    z = torch.zeros
    with pytest.raises(SgrError):
        GaussianRasterizer(st)(z(4, 3), None, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(SgrError):
        distCUDA2(z(10, 3))
    with pytest.raises(SgrError):
        losses.ssim(z(3, 8, 8), z(3, 8, 8))
    with pytest.raises(SgrError):
        scene.compose([scene.Segment(z(2, 3), z(2, 4), z(2, 3), z(2, 1), z(2, 1, 3), z(2, 15, 3))], 16, 0)


def test_host_only_entry_points_answer_without_a_gpu(lib):
    """The entry points that only read or set process-wide host state make no HIP call: the ABI version (bumped whenever a
    struct of include/sgr.h grows: sgr_backward_extras), whether the A/B designs are compiled in (not in the shipped build),
    and the lazy switch (query, set, restore; its status call reports that no lazy forward has run on this thread)."""
    lib.sgr_version.restype = C.c_int
    assert lib.sgr_version() >= 101
    assert lib.sgr_has_variants() == 0
    prev = lib.sgr_set_lazy(-1)
    assert prev in (0, 1)
    assert lib.sgr_set_lazy(1) == prev
    assert lib.sgr_set_lazy(-1) == 1
    r, c, f = C.c_int(), C.c_int(), C.c_int()
    assert lib.sgr_lazy_status(C.byref(r), C.byref(c), C.byref(f)) < 0
    lib.sgr_last_error.restype = C.c_char_p
    assert b"lazy" in lib.sgr_last_error()
    lib.sgr_set_lazy(prev)
    assert lib.sgr_set_lazy(-1) == prev


def test_cross_file_launchers_are_declared_in_one_header_only():
    """Every launcher one kernel source defines and another calls is declared in csrc/sgr_launch.h, which the defining
    file includes too: no .hip file carries a prototype (a declaration ending in `;`) of its own that could go stale.  The
    header is a build dependency (build.HEADERS: objects rebuild, source_sha16 sees it) and declares them."""
    from street_gaussians_amd import build
    proto = re.compile(r"^[A-Za-z_][\w \t\*&:<>]*?\b(sgr_launch_\w+|sgr_knn_impl|sgr_partial_row_stride)\s*\([^;{}]*\)\s*;", re.M)
    stale = {}
    for path in sorted(glob.glob(os.path.join(build.CSRC, "**", "*.hip"), recursive=True)):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
        names = [m.group(1) for m in proto.finditer(text)]  # (at column 0: a call is indented, a definition ends in `{`)
        if names:
            stale[os.path.relpath(path, build.CSRC)] = names
    assert not stale, stale
    assert "sgr_launch.h" in build.HEADERS
    header = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(build.CSRC, "sgr_launch.h")).read(), flags=re.S)
    declared = {m.group(1) for m in proto.finditer(header)}
    assert {"sgr_launch_preprocess", "sgr_launch_blend_fwd", "sgr_launch_blend_bwd", "sgr_launch_blend_bwd_sw",
            "sgr_knn_impl", "sgr_partial_row_stride"} <= declared, sorted(declared)
    assert re.search(r"\bsgr_launch_gauss_bwd\s*,\s*sgr_launch_gauss_bwd_strict\s*;", header)  # one declaration, both names


SW_ENUM = re.compile(r"^\s*SGR_SW_(\w+)\s*=\s*1\s*<<\s*(\d+)\s*,?", re.M)
VARIANT_BITS = (1 << 4) | (1 << 5) | (1 << 8) | (1 << 9)  # USE_V2, USE_ONESWEEP, USE_SW, USE_RS_WAVE


def _switch_enum():
    return [(name, int(bit)) for name, bit in SW_ENUM.findall(open(os.path.join(ROOT, "include", "sgr.h")).read())]


def test_switch_enum_covers_every_bit_and_the_binding_agrees():
    """The SGR_SW_* enum of include/sgr.h names bits 0..18, one entry each, and street_gaussians_amd._C carries the same
    names (without the prefix) with the same values -- bench.py, the tests and the tools use the Python names."""
    from street_gaussians_amd import _C
    enum = _switch_enum()
    assert sorted(bit for _, bit in enum) == list(range(19)), enum
    assert len({name for name, _ in enum}) == len(enum)
    for name, bit in enum:
        assert getattr(_C, name) == 1 << bit, name
    # the names the callers use, every one of them in the enum
    assert {name for name, _ in enum} == {"NO_CULL", "NO_DPP", "NO_DET", "NO_HITS", "USE_V2", "USE_ONESWEEP", "PRE_STAGE_SH",
                                          "EXACT", "USE_SW", "USE_RS_WAVE", "REF_RECT", "NO_TILE_MASK", "TILE_SORT",
                                          "REF_RECT_PLAIN", "LPT", "NO_LPT", "NO_HLIST", "HLIST_ALWAYS", "KEY32"}


def test_test_switches_round_trips_every_bit(lib):
    """sgr_test_switches sets and reports every bit; a library without the A/B variants drops their bits (4, 5, 8, 9).
    Host state only: no HIP call is made."""
    variants = lib.sgr_has_variants() != 0
    prev = lib.sgr_test_switches(-1)
    try:
        for bit in range(19):
            m = 1 << bit
            lib.sgr_test_switches(m)
            want = m if (variants or not m & VARIANT_BITS) else 0
            assert lib.sgr_test_switches(-1) == want, bit
        lib.sgr_test_switches(0)
        assert lib.sgr_test_switches(-1) == 0
        everything = (1 << 19) - 1
        lib.sgr_test_switches(everything)
        assert lib.sgr_test_switches(-1) == (everything if variants else everything & ~VARIANT_BITS)
    finally:
        lib.sgr_test_switches(prev)
    assert lib.sgr_test_switches(-1) == prev


# every environment name of the initial mask, aliases included (SGR_ONESWEEP is the radix sort's own flag: bit 5)
SWITCH_ENV = {"SGR_NO_CULL": 0, "SGR_NO_DPP": 1, "SGR_NO_DET": 2, "SGR_NO_HITS": 3, "SGR_V2": 4, "SGR_ONESWEEP": 5,
              "SGR_PRE_STAGE": 6, "SGR_EXACT": 7, "SGR_SW": 8, "SGR_SW8": 8, "SGR_RS_WAVE": 9, "SGR_SW9": 9,
              "SGR_REF_RECT": 10, "SGR_NO_TILE_MASK": 11, "SGR_TILE_SORT": 12, "SGR_REF_RECT_PLAIN": 13, "SGR_LPT": 14,
              "SGR_NO_LPT": 15, "SGR_NO_HLIST": 16, "SGR_HLIST_ALWAYS": 17, "SGR_KEY32": 18}


def test_switch_environment_names_set_the_initial_mask(lib):
    """A fresh process with exactly one of the names set (to 1) starts with exactly that bit -- or with none, for a variant bit
    in a library without the variants; with none of them set the mask starts at 0 (`_C.test_switches(-1)`: host only)."""
    import subprocess
    import sys
    from concurrent.futures import ThreadPoolExecutor
    variants = lib.sgr_has_variants() != 0
    base = {k: v for k, v in os.environ.items() if k not in SWITCH_ENV}
    code = "from street_gaussians_amd import _C; print(_C.test_switches(-1))"

    def initial_mask(name):
        env = dict(base, **({name: "1"} if name else {}))
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        return int(r.stdout.split()[-1])

    cases = [(None, 0)] + [(name, 1 << bit) for name, bit in SWITCH_ENV.items()]
    with ThreadPoolExecutor(4) as pool:
        got = list(pool.map(initial_mask, [name for name, _ in cases]))
    for (name, m), g in zip(cases, got):
        assert g == (m if (variants or not m & VARIANT_BITS) else 0), (name, g)


def test_export_table_lists_every_array_the_header_names():
    """`_C._EXPORT` (the names tests read internal arrays by) against the `which` numbers of sgr_export_internal's comment in
    include/sgr.h: every array the header names has a row, cov3D (3, the one sgr_export_cov3d recomputes) included."""
    import re
    from street_gaussians_amd import _C
    text = open(os.path.join(ROOT, "include", "sgr.h")).read()
    block = text[text.index("* which: 0 depths"):text.index("int sgr_export_internal(")]
    named = {int(m) for m in re.findall(r"(?:which: |\| |\* {8})(\d+) (?=[a-z])", block)}
    assert named == {v[0] for v in _C._EXPORT.values()}, sorted(named)
    which, dtype, shape = _C._EXPORT["cov3D"]
    assert which == 3 and shape(7, 0, 0, 0) == (7, 6) and "sgr_export_cov3d" in block
