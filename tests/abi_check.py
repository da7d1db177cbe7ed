"""What every check of the C surface shares (a plain helper module, imported as the *_ref.py modules are): a reading of the headers
under include/ (symbols, parameter kinds, return types, struct fields), the kinds of a ctypes binding, the literal `lib.call` names
of a piece of Python, the build-if-missing library, and the census of a launcher family.  tests/test_abi.py holds every pair of
diffcodec_amd.lib.ABI to its header with these; a family's own test module keeps only what is specific to the family."""
import ast
import ctypes
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETURN_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
_KINDS = {ctypes.c_void_p: "p", ctypes.c_int: "int", ctypes.c_longlong: "long", ctypes.c_float: "float", ctypes.c_double: "double"}


@functools.lru_cache(maxsize=None)
def header_source(header):
    """the text of include/<header> without its comments, /* */ and //"""
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def header_symbols(header):
    """the sorted dc_* function names include/<header> declares"""
    return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", header_source(header))))


def _kind(decl):
    """'p' for a pointer declarator, else the word before its name: 'int' | 'long' (long long) | 'float' | 'double'"""
    return "p" if "*" in decl else decl.split()[-2]


def _declaration(src, name):
    m = re.search(r"\b(int|long long)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name}: no declaration returning int or long long"
    return m


def arg_kinds(src, name):
    """the kind of each parameter of `name` as declared in the comment-free header text `src`; [] for (void)"""
    args = [" ".join(a.split()) for a in _declaration(src, name).group(2).split(",")]
    return [] if args == ["void"] else [_kind(a) for a in args]


def return_kind(src, name):
    """'int' | 'long long'"""
    return _declaration(src, name).group(1)


def binding_kinds(argtypes):
    """the kinds of a table entry; a POINTER(...) type is a pointer"""
    return [_KINDS.get(a, "p") for a in argtypes]


def struct_fields(src, struct):
    """[(field name, kind)] of `typedef struct <struct> { ... } <struct>;` in declaration order"""
    body = src[src.index("typedef struct " + struct + " {"):src.index("} " + struct + ";")].split("{", 1)[1]
    fields = []
    for stmt in (" ".join(s.split()) for s in body.split(";")):
        if not stmt:
            continue
        first, *more = stmt.split(",")
        fields.append((re.findall(r"\w+", first)[-1], _kind(first)))
        scalar = first.split()[-2]                                  # `int N, H, W`: the later declarators share the type
        fields += [(re.findall(r"\w+", d)[-1], "p" if "*" in d else scalar) for d in more]
    return fields


def lib_calls(source, attr="call"):
    """C names that are the literal first argument of a `lib.call(...)` expression in Python source text (from the syntax tree: a
    name in a comment or in an unused string does not count); attr="query": of a `lib.query(...)` expression"""
    names = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == attr and \
                isinstance(node.func.value, ast.Name) and node.func.value.id == "lib" and node.args and \
                isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str):
            names.add(node.args[0].value)
    return names


def module_source(module):
    """the text of tests/<module>.py"""
    return open(os.path.join(ROOT, "tests", module + ".py")).read()


def built_lib():
    """diffcodec_amd.lib, with the shared object built first when it is missing"""
    import __graft_entry__ as g
    from diffcodec_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return lib


def family_census(signatures, queries, tests_source, product_source):
    """-> (launchers of `signatures` with no literal lib.call in either source, queries the product source never names).  `queries`
    return a size or fill a route, not a launch status: the product asks them as `lib.load().<name>(` or through lib.query."""
    called = lib_calls(tests_source) | lib_calls(product_source)
    uncalled = sorted(set(signatures) - set(queries) - called)
    asked = lib_calls(product_source, "query")
    unnamed = sorted(q for q in queries if q in signatures and (q + "(") not in product_source and q not in asked)
    return uncalled, unnamed
