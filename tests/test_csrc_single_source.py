"""The split-bf16 contract and the shared tile helpers are written once: csrc/split_bf16.h and csrc/dif_common.h.  So is the
host side of a launch: csrc/dif_launch.h (launch + status, the dynamic-LDS attribute) and csrc/dif_select.h (variant selectors).
Reads the device sources as text (no compiler, no GPU) so that the per-file copies cannot grow back."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difformer_amd", "csrc")
HOMES = ("split_bf16.h", "dif_common.h")
SHARED = ("zero4", "split_bf16", "split8", "cat8", "mfma3", "dinv_of", "tile_product", "ld4", "ld4_raw", "mask4", "sigmoid_hw")

# `typedef __bf16 name __attribute__((ext_vector_type(n)))`, `using name = __bf16 __attribute__((...))`, and the same through
# the other spellings of the element type
BF16_VECTOR = re.compile(r"\b(?:typedef\s+(?:__bf16|__hip_bfloat16|hip_bfloat16)\b[^;]*vector_type|using\s+\w+\s*=\s*(?:__bf16|__hip_bfloat16|hip_bfloat16)\b[^;]*vector_type)")


def sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, name)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            out[name] = re.sub(r"//[^\n]*", "", text)
    return out


def definitions(text, name):
    """Free functions called `name` that have a body.  A definition is `<qualifiers and return type> name(<parameters>) {`
    with a device / inline qualifier in front; the static member functions of dif::Elem<T> (ld4 among them) are not meant."""
    found = []
    for m in re.finditer(r"^[^\n;=(]*\b(?:__device__|__host__|__forceinline__|inline)\b[^\n;=(]*[\s&*]%s\s*\(" % re.escape(name), text, flags=re.M):
        if re.search(r"\bstatic\b", m.group(0)):
            continue
        depth, i = 1, m.end()
        while depth:                            # the matching parenthesis of the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        if re.match(r"\s*(?:const\s*)?\{", text[i:]):
            found.append(m.group(0).strip())
    return found


def test_the_sources_are_where_the_test_looks():
    src = sources()
    assert set(HOMES) <= set(src) and len([n for n in src if n.endswith(".hip")]) >= 25


def test_bf16_vector_types_are_declared_in_split_bf16_h_only():
    src = sources()
    assert len(BF16_VECTOR.findall(src["split_bf16.h"])) == 2            # bf16x4, bf16x8
    offenders = {n: BF16_VECTOR.findall(t) for n, t in src.items() if n != "split_bf16.h" and BF16_VECTOR.search(t)}
    assert not offenders, offenders


def test_no_kernel_file_defines_a_shared_helper():
    offenders = {(n, name): d for n, t in sources().items() if n not in HOMES for name in SHARED for d in [definitions(t, name)] if d}
    assert not offenders, offenders


def test_every_shared_helper_is_defined_exactly_once():
    src = sources()
    counts = {name: sum(len(definitions(src[h], name)) for h in HOMES) for name in SHARED}
    assert counts == {name: 1 for name in SHARED}, counts


def test_the_radix_pass_kernels_are_launched_from_one_place():
    """csrc/gcn_csr.hip: every sort of the graph construction goes through the one pass loop."""
    text = sources()["gcn_csr.hip"]
    assert text.count('dif::launch("radix_hist_kernel", radix_hist_kernel,') == 1
    assert text.count('dif::launch("radix_scatter_kernel", radix_scatter_kernel,') == 1
    assert len(re.findall(r"\bradix_hist_kernel\s*,", text)) == 1 and len(re.findall(r"\bradix_scatter_kernel\s*,", text)) == 1


LAUNCH_HOME = "dif_launch.h"
SIDE_LIBRARIES = ("attn_topk.hip", "attn_edges.hip")      # their own shared objects, their own last-error text
LAUNCH = re.compile(r"\bhipLaunchKernelGGL\b|<<<|\bdif::launch\s*\(|\bhipLaunchKernel\b|\bhipModuleLaunchKernel\b")


def function_like_macros(text):
    """[(name, body)] of every `#define NAME(...) body`, continuation lines joined"""
    return [(m.group(1), m.group(2).replace("\\\n", " "))
            for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)\([^)]*\)((?:[^\n\\]|\\\n|\\.)*)", text, flags=re.M)]


def test_no_macro_expands_to_a_kernel_launch():
    """A launcher turns run-time facts into template arguments with dif::with_flags / dif::with_int, not with a private macro."""
    offenders = {(n, name) for n, t in sources().items() for name, body in function_like_macros(t) if LAUNCH.search(body)}
    assert not offenders, offenders


def test_the_lds_attribute_is_set_in_one_place():
    assert [n for n, t in sources().items() if "hipFuncSetAttribute" in t] == [LAUNCH_HOME]


def test_kernels_are_launched_through_the_launch_helper():
    """libdifformer_hip.so: dif::launch only.  The two side libraries keep their own status check and launch directly."""
    users = sorted(n for n, t in sources().items() if "hipLaunchKernelGGL" in t or "<<<" in t)
    assert users == sorted((LAUNCH_HOME,) + SIDE_LIBRARIES), users
    assert sources()[LAUNCH_HOME].count("hipLaunchKernelGGL(") == 1


def test_the_macro_finder_sees_a_launch_macro():
    text = "#define DIF_X(G, V)  \\\n    do { \\\n        hipLaunchKernelGGL((k<G, V>), grid, block, 0, st, a); \\\n    } while (0)\n#define DIF_Y(c) ((c) + 1)\n"
    found = dict(function_like_macros(text))
    assert set(found) == {"DIF_X", "DIF_Y"} and LAUNCH.search(found["DIF_X"]) and not LAUNCH.search(found["DIF_Y"])
    assert LAUNCH.search("return dif::launch(\"k\", k<G>, grid, block, 0, st);") and LAUNCH.search("k<<<g, b, 0, st>>>(a);")


def test_the_sort_rounds_formula_is_written_once():
    assert sources()["gcn_csr.hip"].count("64 * 4096") == 1


def test_the_definition_finder_sees_a_copy():
    copy = "namespace {\ntemplate <bool VEC>\n__device__ __forceinline__ f32x4 ld4(const float* __restrict__ base, int64_t ld,\n   int width) {\n    return f32x4{};\n}\n}"
    assert len(definitions(copy, "ld4")) == 1 and not definitions(copy, "ld4_raw")
    assert not definitions("    z = ld4<VEC>(base, ld, rc, rok, col0, c, width);\n    if (x) split8(a, b, hi, lo);", "ld4")
    assert BF16_VECTOR.search("typedef __bf16 my8 __attribute__((ext_vector_type(8)));")
    assert BF16_VECTOR.search("using my8 = __bf16 __attribute__((ext_vector_type(8)));")
