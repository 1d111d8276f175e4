"""The plumbing of the long-list metric launch without a GPU: the header declares ultr_metrics_long / ultr_metrics_max_list, _lib binds
them with ultr_metrics_report's argument list, the ABI stays 8, and engine.metrics_fit follows the library's bound while the 64 KiB rule
of the one-wave kernel keeps its own function."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    from ultra_pytorch_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_header_and_binding_carry_the_two_entries():
    from ultra_pytorch_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ultr_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint ultr_metrics_long\(const float\* scores,", hdr)
    assert re.search(r"\bint32_t ultr_metrics_max_list\(void\);", hdr)
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    assert _lib.SIGNATURES["ultr_metrics_long"] == _lib.SIGNATURES["ultr_metrics_report"]
    assert _lib.SIGNATURES["ultr_metrics_max_list"][1] == []
    lib = _library()
    assert lib.ultr_abi_version() == 8
    assert hasattr(lib, "ultr_metrics_long") and hasattr(lib, "ultr_metrics_max_list")


def test_the_bound_takes_4096_and_fits_160_kib():
    mx = int(_library().ultr_metrics_max_list())
    assert mx >= 4096
    # five float arrays and a validity bit per document: no more than 160 KiB hold (8141 documents), and within 2 % of that
    assert 20 * mx + mx // 8 <= 160 * 1024 and mx >= 0.98 * 8141


def test_metrics_fit_is_the_library_s_bound():
    from ultra_pytorch_amd import engine
    mx = int(_library().ultr_metrics_max_list())
    assert engine.metrics_fit(mx) and not engine.metrics_fit(mx + 1)
    assert engine.metrics_fit(1) and engine.metrics_fit(813) and engine.metrics_fit(814) and engine.metrics_fit(1251)
    assert not engine.metrics_fit(0)


def test_the_one_wave_kernel_keeps_its_own_rule():
    from ultra_pytorch_amd import engine
    assert engine.metrics_fit_short(1) and engine.metrics_fit_short(813) and not engine.metrics_fit_short(814)
    assert engine.ndcg_fit(1023) and not engine.ndcg_fit(1024)
