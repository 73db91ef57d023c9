"""The C-ABI library loads without a GPU and exports exactly what include/gsr.h declares, with the
argument counts and struct layouts the ctypes binding uses (no compute calls: no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

from diff_gaussian_rasterization import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsr.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*(?:const\s+)?[\w\s\*]+?\b(gsr_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        out[name] = n
    return out


def test_header_parses():
    fns = header_functions()
    for required in ("gsr_forward_preprocess", "gsr_num_rendered", "gsr_forward_render", "gsr_backward",
                     "gsr_mark_visible", "gsr_geom_bytes", "gsr_binning_bytes", "gsr_image_bytes",
                     "gsr_backward_bytes", "gsr_version", "gsr_last_error", "gsr_profile_enable",
                     "gsr_profile_read"):
        assert required in fns, required


def test_library_exports_every_declared_symbol():
    lib = _C.load_library()
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in gsr.h but not exported"


def test_binding_signatures_match_header():
    fns = header_functions()
    assert set(fns) == set(_C.SIGNATURES), set(fns) ^ set(_C.SIGNATURES)
    for name, nargs in fns.items():
        assert len(_C.SIGNATURES[name][1]) == nargs, f"{name}: header {nargs} args, binding {len(_C.SIGNATURES[name][1])}"


def header_struct_fields():
    """{struct name: [field names in order]} of the header's `typedef struct NAME { ... } NAME;` blocks."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", src, flags=re.S):
        names = []
        for decl in m.group(2).split(";"):
            # declarators after the type: the last identifier of each comma-separated piece
            names += [re.findall(r"\w+", piece)[-1] for piece in decl.split(",") if re.search(r"\w", piece)]
        out[m.group(1)] = names
    return out


def test_struct_layouts_match_header(tmp_path):
    """The ctypes structures of the view-set calls against the header's, through the C compiler: the same field
    names, and for each the same offset, and the same size.  (An argument count says nothing about a struct
    pointer; two fields swapped on one side would pass it.)  Compiling the header as C also proves it is C."""
    declared = header_struct_fields()
    assert set(declared) == set(_C.STRUCTS)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gsr.h"', "int main(void) {"]
    for name, cls in _C.STRUCTS.items():
        fields = [f[0] for f in cls._fields_]
        assert fields == declared[name], name
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    want = {}
    for name, cls in _C.STRUCTS.items():
        want[name] = str(ctypes.sizeof(cls))
        for f in cls._fields_:
            want[f"{name}.{f[0]}"] = str(getattr(cls, f[0]).offset)
    assert got == want


def test_host_only_queries():
    lib = _C.load_library()
    assert lib.gsr_abi_version() == _C.ABI_VERSION
    assert lib.gsr_version().decode().startswith("gsr ")
    assert "gfx950" in lib.gsr_version().decode()
    assert lib.gsr_geom_bytes(1000) >= 1000 * (48 + 8 + 4 * 7)  # records, rect, 7 u32 words
    assert lib.gsr_set_geom_bytes(4, 1000) >= 4 * lib.gsr_geom_bytes(1000) - 4 * 4096
    assert lib.gsr_binning_bytes(5000, 64, 64) >= 5000 * 16
    assert lib.gsr_image_bytes(64, 48) >= 64 * 48 * 8
    assert lib.gsr_backward_bytes(10, 100) >= 100 * 48 + 10 * 13 * 4  # one row per instance + per-Gaussian records
    assert lib.gsr_geom_bytes(0) > 0  # sizes stay valid for P = 0


def test_argument_errors_without_gpu():
    """Argument validation happens before any device work and reports the reference's messages."""
    lib = _C.load_library()
    v = ctypes.c_void_p(16)  # never dereferenced: the call must fail validation first
    rc = lib.gsr_forward_preprocess(10, 0, 1, v, v, 1.0, v, v, v, v, None, v, v, v, 64, 64, 0.5, 0.5, 0,
                                    v, v, None)
    assert rc == 1
    assert b"exactly one of either SHs or precomputed colors" in lib.gsr_last_error()
    rc = lib.gsr_forward_preprocess(10, 0, 1, v, None, 1.0, v, v, v, None, v, v, v, v, 64, 64, 0.5, 0.5, 0,
                                    v, v, None)
    assert rc == 1
    assert b"scale/rotation pair or precomputed 3D covariance" in lib.gsr_last_error()
    assert lib.gsr_forward_render(1, 1, 0, 64, v, v, v, v, v, v, v, None) == 1

    # the view-set calls: each rule that selects a variant by its fields is checked before any device work too
    a = 16  # (never dereferenced either)
    K = (ctypes.c_int * 1)(100)
    ptrs = (ctypes.c_void_p * 1)(a)
    tan = (ctypes.c_float * 1)(0.5)
    scene = _C.SetScene(V=1, P=10, degree=0, M=1, width=64, height=64, scale_modifier=1.0, means3D=a, scales=a,
                        rotations=a, opacities=a, shs=a, viewmatrices=ptrs, projmatrices=ptrs, campos=ptrs, bgs=ptrs,
                        tanfovx=tan, tanfovy=tan)
    state = _C.SetState(radii=a, geom=a, binning=a, image=a, num_rendered=K)

    def err(rc):
        assert rc == 1
        return lib.gsr_last_error()

    both = _C.SetScene.from_buffer_copy(scene)
    both.colors_precomp = a
    assert b"exactly one of either SHs or precomputed colors" in err(lib.gsr_set_preprocess(both, state, None, None))
    nocov = _C.SetScene.from_buffer_copy(scene)
    nocov.scales = None
    assert b"scale/rotation pair or precomputed 3D covariance" in err(
        lib.gsr_set_preprocess(nocov, state, None, None))

    out = dict(out_color=a, out_depth=a, out_alpha=a)
    assert b"composite needs out_render" in err(
        lib.gsr_set_render(scene, state, _C.SetOutputs(bg_images=a, **out), None))
    assert b"null second colour argument" in err(
        lib.gsr_set_render(scene, state, _C.SetOutputs(colors2=a, **out), None))
    assert b"null second colour argument" in err(
        lib.gsr_set_render(scene, state, _C.SetOutputs(out_color2=a, **out), None))

    g = dict(dL_dcolor=a, dL_dmeans2D=a, dL_dcolors=a, dL_dopacity=a, dL_dmeans3D=a, dL_dcov3D=a, dL_dsh=a,
             dL_dscales=a, dL_drotations=a, work=a, work_bytes=1 << 30)

    def backward(sc=scene, **fields):
        return err(lib.gsr_set_backward(sc, state, _C.SetGrads(**dict(g, **fields)), None))

    assert b"composite needs the forward's color" in backward(bg_images=a)
    assert b"dL_dbg needs bg_images" in backward(color=a, dL_dbg=a)
    two = b"two-colour backward needs colors2, dL_dcolor2 and dL_dcolors2"
    for given in (("colors2",), ("dL_dcolor2",), ("dL_dcolors2",), ("colors2", "dL_dcolor2"),
                  ("colors2", "dL_dcolors2"), ("dL_dcolor2", "dL_dcolors2")):
        assert two in backward(**{k: a for k in given}), given
    nosh = _C.SetScene.from_buffer_copy(scene)
    nosh.shs = None
    assert two in backward(nosh, colors2=a, dL_dcolor2=a, dL_dcolors2=a, colors_override=a, dL_dsh=None)
    override = b"colors_override excludes SHs and the depth / alpha gradients"
    assert override in backward(colors_override=a, dL_dsh=None)  # (the scene has SHs)
    assert override in backward(nosh, colors_override=a)  # (dL_dsh given)
    assert override in backward(nosh, colors_override=a, dL_dsh=None, dL_ddepth=a)
    assert override in backward(nosh, colors_override=a, dL_dsh=None, dL_dalpha=a)
    chunks = b"bad gradient chunk request"
    events = (ctypes.c_void_p * 17)()
    GSR_GRAD_CHUNKS_MAX = 16
    assert chunks in backward(n_chunks=GSR_GRAD_CHUNKS_MAX + 1, chunk_events=events)
    assert chunks in backward(n_chunks=-1)
    assert chunks in backward(n_chunks=1, chunk_events=None)
    assert b"accumulate needs dL_dcov3D" in backward(accumulate=1, dL_dcov3D=None)

    # SH rows wider than k_gauss_accum can stage in the CU's 160 KB of LDS (256 rows of sh_lds_stride(M) floats plus
    # s_rl and s_wcnt: M = 50 asks for 160 016 bytes, M = 51 for 164 112) are rejected before any launch, by the
    # preprocess and by the backward; M = 50 passes that check and fails the next one
    import gauss_backward_cases as gc

    assert gc.max_sh() == 50
    wide = _C.SetScene.from_buffer_copy(scene)
    wide.M = gc.max_sh() + 1
    limit = b"largest SH width the per-Gaussian backward's LDS staging holds: M <= 50"
    assert limit in err(lib.gsr_set_preprocess(wide, state, None, None))
    assert limit in backward(wide)
    nocounts = _C.SetState(radii=a, geom=a, binning=a, image=a, num_rendered=None)
    fits = _C.SetScene.from_buffer_copy(scene)
    fits.M = gc.max_sh()
    assert b"null pointer argument" in err(lib.gsr_set_backward(fits, nocounts, _C.SetGrads(**g), None))
    wide.colors_precomp, wide.shs = a, None  # (M is ignored without SHs)
    assert b"null pointer argument" in err(lib.gsr_set_backward(wide, nocounts, _C.SetGrads(**dict(g, dL_dsh=None)), None))

    assert lib.gsr_set_backward_bytes(1, 10, K, 0) > 0
    for two_colors in (0, 1):
        assert lib.gsr_set_backward_bytes(0, 10, K, two_colors) == 0
        assert lib.gsr_set_backward_bytes(65, 10, K, two_colors) == 0
        assert lib.gsr_set_backward_bytes(1, 10, None, two_colors) == 0


def test_oracle_library_builds_and_exports():
    import oracle

    lib = oracle.lib()
    for name in ("oracle_forward_f32", "oracle_forward_f64", "oracle_backward_f32", "oracle_backward_f64",
                 "oracle_eval_sh_f64", "oracle_cov3d_f64"):
        assert hasattr(lib, name)


def test_image_bytes_follow_the_split_decision(monkeypatch):
    """gsr_set_image_bytes sizes the image buffer for the forward's split decision: with the split backward's
    checkpoints (335 MB for one 1024^2 view) only when the forward writes them (one colour set, quadrant waves,
    GSR_BWD_SPLIT not 0); without counts (NULL) it is the upper bound."""
    import ctypes

    lib = _C.load_library()
    K = (ctypes.c_int * 1)(5000)
    full = lib.gsr_set_image_bytes(1, 1000, None, 1024, 1024, 0)
    monkeypatch.delenv("GSR_BWD_SPLIT", raising=False)
    monkeypatch.delenv("GSR_FWD_KERNEL", raising=False)
    split = lib.gsr_set_image_bytes(1, 1000, K, 1024, 1024, 0)
    two = lib.gsr_set_image_bytes(1, 1000, K, 1024, 1024, 1)
    assert split == full and two < full and full - two >= 4096 * 16 * 5 * 256 * 4 - 256
    monkeypatch.setenv("GSR_BWD_SPLIT", "0")
    assert lib.gsr_set_image_bytes(1, 1000, K, 1024, 1024, 0) == two
    K64 = (ctypes.c_int * 64)(*([5000] * 64))
    assert (lib.gsr_set_image_bytes(64, 1000, K64, 1024, 1024, 0)
            == lib.gsr_set_image_bytes(64, 1000, None, 1024, 1024, 0))
