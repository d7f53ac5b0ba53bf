"""CPU tests of the C-ABI boundary: liboflk.so loads without a GPU, exports every
symbol include/oflk.h declares, and its host-only helpers behave.  No compute
entry point is called here."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def declared_functions():
    text = (ROOT / "include" / "oflk.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oflk_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_reference_surface():
    names = declared_functions()
    for must in ["oflk_compute_gradients", "oflk_from_gradients", "oflk_single_scale", "oflk_build_pyramid",
                 "oflk_warp", "oflk_upsample_flow", "oflk_pyramidal", "oflk_pyramidal_batch", "oflk_plan_create",
                 "oflk_plan_pyramidal", "oflk_last_error"]:
        assert must in names


def test_library_exports_every_declared_symbol():
    import _oflk

    L = _oflk.lib()
    for name in declared_functions():
        assert hasattr(L, name), f"{name} declared in include/oflk.h but not exported"
        assert name in _oflk.SIGNATURES, f"{name} has no ctypes signature in _oflk.py"
    assert set(_oflk.SIGNATURES) == set(declared_functions())


def declarations():
    """{name: (return class, [parameter classes])} of every function include/oflk.h declares; a class is one of pointer,
    int, unsigned, float, double, size_t, long, void"""
    text = (ROOT / "include" / "oflk.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)       # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{', "", text)

    def kind(decl):
        decl = decl.strip()
        if "*" in decl:
            return "pointer"
        words = [w for w in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl) if w != "const"]
        assert words, decl
        if words[0] == "unsigned":
            assert words[1:2] != ["char"] and words[1:2] != ["long"], decl
            return "unsigned"
        assert words[0] in ("int", "float", "double", "size_t", "long", "void"), decl
        return words[0]

    out = {}
    for stmt in text.split(";"):
        m = re.search(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(oflk_[a-z0-9_]+)\s*\(([^()]*)\)\s*$", stmt, flags=re.S)
        if not m or "typedef" in m.group(1):
            continue
        params = m.group(3).strip()
        out[m.group(2)] = (kind(m.group(1)), [] if params in ("", "void") else [kind(p) for p in params.split(",")])
    return out


def ctypes_class(t):
    """the class of a ctypes restype / argtypes entry, in the words of declarations()"""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    plain = {ctypes.c_int: "int", ctypes.c_uint: "unsigned", ctypes.c_float: "float", ctypes.c_double: "double",
             ctypes.c_size_t: "size_t", ctypes.c_long: "long"}
    return plain[t]


def test_every_signature_has_the_classes_of_its_declaration():
    """SIGNATURES against the header, type by type: the return type and every parameter, position by position, fall in the
    same class (pointer, int, unsigned, float, double, size_t, long, void) as the declaration's"""
    import _oflk

    decl = declarations()
    assert set(decl) == set(declared_functions()) == set(_oflk.SIGNATURES)
    for name, (res, args) in _oflk.SIGNATURES.items():
        got = (ctypes_class(res), [ctypes_class(a) for a in args])
        assert got == decl[name], f"{name}: ctypes {got}, header {decl[name]}"


def test_version_and_device_count_never_fail():
    import _oflk

    assert _oflk.version().startswith("oflk ")
    assert _oflk.device_count() >= 0


def test_stage_predicates_are_declared_and_answer_without_a_device():
    """oflk_upsample_staged / oflk_pyramid_step_fused: host-only like oflk_tolerant_relaxes, 0 or 1 for any arguments
    (what they decide is tested in tests/test_stages_cpu.py)"""
    import _oflk

    L = _oflk.lib()
    assert {"oflk_upsample_staged", "oflk_pyramid_step_fused"} <= set(declared_functions())
    assert L.oflk_upsample_staged(540, 960, 1080, 1920) == 1 and L.oflk_upsample_staged(240, 320, 240, 320) == 0
    assert L.oflk_pyramid_step_fused(1080, 1920, 540, 960, 8) == 1 and L.oflk_pyramid_step_fused(1080, 1920, 648, 1152, 7) == 0
    for args in ((0, 0, 0, 0), (-5, 3, 7, 9), (1 << 30, 1 << 30, 1, 1)):
        assert L.oflk_upsample_staged(*args) in (0, 1)
        assert L.oflk_pyramid_step_fused(*args, 8) in (0, 1)


@pytest.mark.parametrize("shape,levels", [((240, 320), 3), ((1080, 1920), 3), ((2160, 3840), 3), ((37, 53), 3),
                                          ((241, 321), 4), ((5, 7), 2)])
def test_level_dims_follow_int_truncation(oracle, shape, levels):
    import lucas_kanade_pyramidal as P

    got = P.pyramid_level_shapes(shape, levels)
    exp = []
    h, w = shape
    for _ in range(levels):
        exp.insert(0, (h, w))
        h, w = int(h * 0.5), int(w * 0.5)  # reference lucas_kanade_pyramidal.py:51-52
    assert got == exp == oracle.pyramid_dims(shape[0], shape[1], levels)


def test_invalid_arguments_raise_value_error():
    import lucas_kanade_pyramidal as P

    with pytest.raises(ValueError):
        P.pyramid_level_shapes((240, 320), 0)
    with pytest.raises(ValueError):
        P.pyramid_level_shapes((2, 2), 3)  # a level would be empty
    with pytest.raises(ValueError):
        P.pyramid_level_shapes((0, 5), 1)


def test_no_cpu_fallback_when_gpu_absent():
    """the product path must fail loudly, not route through any CPU code"""
    import _oflk
    import lucas_kanade_core as K

    if _oflk.device_count() > 0:
        pytest.skip("a GPU is visible here")
    a = np.zeros((16, 16), np.float32)
    with pytest.raises(_oflk.OflkError) as e:
        K.lucas_kanade_single_scale(a, a)
    assert e.value.code == _oflk.OFLK_ERR_NO_DEVICE and "no CPU path" in str(e.value)


def test_product_modules_never_touch_the_oracle():
    for f in (ROOT / "optical-flow-fpga_amd").rglob("*"):
        if f.suffix in (".py", ".hip", ".hpp", ".cpp", ".h") and f.is_file():
            text = f.read_text()
            assert "oflk_oracle" not in text and "liboflk_oracle" not in text, f


def test_product_translation_unit_carries_no_development_switches():
    """the shipped library reads no environment variable and its translation unit has no build switches: no timing /
    ablation / diagnostic code, no preprocessor conditional, no macro besides OFLK_API and HIP_TRY, and a Makefile that
    passes no -D"""
    import re

    csrc = ROOT / "optical-flow-fpga_amd" / "csrc"
    sources = sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.hpp"))
    assert {"oflk.hip", "oflk_kernels.hpp", "oflk_stream.hpp"} <= {f.name for f in sources}
    for f in sources:
        text = f.read_text()
        assert "getenv" not in text, f.name
        for word in ("OFLK_ABLATE", "OFLK_LK16_ABL", "OFLK_LK16_TILED", "OFLK_LK16_COLS", "OFLK_TPB", "OFLK_X_", "k_lk16s",
                     "k_lk16<", "OFLK_DIAG", "OFLK_STAMP", "OFLK_PROBE", "OFLK_LKS_ABL"):
            assert word not in text, (f.name, word)
        for n, line in enumerate(text.splitlines(), 1):
            assert not re.match(r"\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", line), (f.name, n, line)
            m = re.match(r"\s*#\s*define\s+(\w+)", line)
            assert not m or m.group(1) in ("OFLK_API", "HIP_TRY"), (f.name, n, line)
    mk = (csrc / "Makefile").read_text()
    assert "DEFS" not in mk
    assert not re.search(r"(?<![\w-])-D", mk), "the Makefile passes no -D"
