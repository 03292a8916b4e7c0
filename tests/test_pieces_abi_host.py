"""The C ABI of the extension header include/poreseg_pieces.h (ps_detect_pieces) -- no GPU compute.  What test_host_logic.py
checks for poreseg.h, for the header beside it: every declared function is exported by libporeseg.so, is in the binding's table
for that header and has the ctypes signature the prototype says; both tables are applied by the one loop of _lib.lib()."""
import os
import re

from test_host_logic import ROOT, ctypes_kind

from pypore_amd import _lib

SCALAR = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "double": "f64", "void": "void"}


def prototypes():
    text = open(os.path.join(ROOT, "include", "poreseg_pieces.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))

    def kind(decl, named):
        if "*" in decl:
            return "ptr"
        words = [w for w in decl.split() if w != "const"]
        assert len(words) == (2 if named else 1), decl
        return SCALAR[words[0]]

    protos = {}
    for statement in re.split(r"[;{}]", text):
        m = re.match(r"\s*([\w\s\*]+?)\b(ps_[a-z_0-9]+)\s*\((.*)\)\s*$", statement, flags=re.S)
        if m:
            protos[m.group(2)] = (kind(m.group(1), False), [kind(p.strip(), True) for p in m.group(3).split(",")])
    return protos


def test_pieces_header_and_binding_agree():
    protos = prototypes()
    assert set(protos) == set(_lib.PIECES_EXPORTS) == {"ps_detect_pieces"}
    assert not set(_lib.PIECES_EXPORTS) & set(_lib.EXPORTS)
    L = _lib.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert [ctypes_kind(t) for t in fn.argtypes] == params and ctypes_kind(fn.restype) == ret, name
    assert protos["ps_detect_pieces"] == ("i32", ["ptr", "ptr", "ptr", "i64", "f64", "ptr", "ptr", "i64", "ptr"])
    assert len(re.findall(r"\.argtypes\s*=", open(_lib.__file__).read())) == 1        # still one place that declares
    assert '#include "poreseg.h"' in open(os.path.join(ROOT, "include", "poreseg_pieces.h")).read()
