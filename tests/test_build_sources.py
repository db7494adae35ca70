"""The build's file lists match csrc/, and the host launchers are declared in one place.

build_ext.SOURCES decides what is compiled and build_ext.HEADERS what an object depends on: a
source missing from the first is never linked, a header missing from the second leaves stale
objects after an edit. csrc/sgm_launch.h is the only declaration of the `launch_*` functions, so
a definition that drifts from it does not compile; a hand-copied prototype elsewhere would bring
back the unchecked second declaration.
"""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd")
CSRC = os.path.join(PKG_DIR, "csrc")


def _build_ext():
    spec = importlib.util.spec_from_file_location("sgm_build_ext_lists", os.path.join(PKG_DIR, "build_ext.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _csrc(*exts):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(exts))


def test_every_source_is_listed():
    assert sorted(_build_ext().SOURCES) == _csrc(".hip", ".cpp")


def test_every_header_is_listed():
    assert sorted(_build_ext().HEADERS) == _csrc(".h")


def test_listed_files_exist():
    be = _build_ext()
    for f in be.SOURCES + be.HEADERS:
        assert os.path.isfile(os.path.join(CSRC, f)), f


# `<type> launch_name(` where the type is not a keyword that starts a call statement
_PROTO = re.compile(r"(?<![\w:])(?!return\b|else\b)[A-Za-z_][\w:<>]*[\s*&]+(launch_\w+)\s*\(")


def _launcher_prototypes(text):
    """Names of the body-less declarations of functions called launch_* in a C++ text."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", text, flags=re.S)
    found = []
    for m in _PROTO.finditer(text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        if re.match(r"\s*;", text[i:]):        # `{` follows a definition, `,` or `)` a call in an expression
            found.append(m.group(1))
    return found


def test_prototype_detector():
    assert _launcher_prototypes("hipError_t launch_a(const Geom&, int np = 8);") == ["launch_a"]
    assert _launcher_prototypes("static void\nlaunch_b(int (*f)(int),\n int);") == ["launch_b"]
    assert _launcher_prototypes("hipError_t launch_c(int v)\n{\n    return launch_d(v);\n}") == []
    assert _launcher_prototypes("if (x) launch_e<4>(v); else launch_f(v); HIP_TRY(sgm::launch_g(v), \"g\");") == []
    assert _launcher_prototypes("// hipError_t launch_h(int);\n") == []


def test_launchers_are_declared_only_in_the_launch_header():
    stray = {}
    for f in _csrc(".hip", ".cpp", ".h"):
        with open(os.path.join(CSRC, f)) as fh:
            names = _launcher_prototypes(fh.read())
        if f == "sgm_launch.h":
            assert len(names) >= 20, f"the launch header declares only {names}"     # 22 when this was written
        elif names:
            stray[f] = names
    assert not stray, f"launcher prototypes outside sgm_launch.h: {stray}"
