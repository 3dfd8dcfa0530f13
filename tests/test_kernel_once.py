"""Every kernel of the library exists once: read from the assembly the build leaves in _obj/<unit>.fixed.s with the parser of scripts/kernel_diff.py.

(a) No two kernel symbols have the same instruction text and .amdhsa_ descriptor once the symbol's own name is substituted out: a kernel copied into a second
    network under another name (the 3 -> 32 RGB first layer and the 4 x 4 NHWC max-pool once were) is the same 500 .. 1000 lines assembled twice.
(b) A symbol sits in one translation unit.  The exception is the template kernels of conv_mfma.h (conv_mfma_h, conv_mfma, gemm_h), whose instantiations the
    units that launch them with their own ConvM each compile; a kernel in an anonymous namespace of a header (conv1a_rgb64 once was) is compiled into every
    unit that includes it.
No GPU needed: hipcc cross-compiles here."""
import importlib.util
import os

from keypoint_bench_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "scripts", "kernel_diff.py"))
kernel_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_diff)


def _kernels():
    build.build()
    if not kernel_diff.kernels(build.OBJ):      # a library that arrived without the _obj/ it was linked from
        build.build(force=True)
    ks = kernel_diff.kernels(build.OBJ)
    assert len(ks) > 200, "the assembly of the build was not found"
    return ks


def test_no_two_kernels_have_the_same_code():
    by_text = {}
    for sym, (norm, _) in _kernels().items():
        assert norm is not None, "%s differs between two units of one build" % sym
        by_text.setdefault(kernel_diff.anonymous(sym, norm), []).append(sym)
    same = sorted(sorted(syms) for syms in by_text.values() if len(syms) > 1)
    assert not same, "the same kernel under more than one name: %s" % same


def test_only_the_conv_mfma_templates_are_compiled_into_more_than_one_unit():
    twice = {sym: sorted(units) for sym, (_, units) in _kernels().items() if len(units) > 1 and not kernel_diff.SHARED_TEMPLATES.search(sym)}
    assert not twice, "kernels compiled into more than one translation unit: %s" % twice
