"""The device eigensolver's size limit, stated in one place per layer: pod.py, the header, the counter table."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as fh:
        return fh.read()


def test_pod_takes_the_device_route_up_to_2048_columns():
    from romtime_amd import pod

    assert pod.DEVICE_EIG_MAX_N == 2048


def test_header_states_the_2048_limit():
    header = _read("include", "romtime_hip.h")
    eig = header[header.index("small symmetric eigenproblem"):header.index("host-side small dense step")]
    assert "3 <= n <= 2048" in eig and "n > 2048 returns RT_ERR_UNSUPPORTED" in eig
    for name in ("rt_sym_eig_values", "rt_sym_eig_values_part", "rt_sym_eig_vectors"):
        assert re.search(r"\b%s\(" % name, eig), name
    pod_orth = header[header.index("The whole of `orth`"):header.index("int rt_pod_orth(")]
    assert "n_cols <= 2048" in pod_orth
    assert "1024 < n <= 2048" in eig        # the wide route is described where its entry points are


def test_wide_form_counter_is_exported_and_documented():
    assert '{"eig_wide_form", RT_CNT_EIG_WIDE_FORM}' in _read("romtime_amd", "csrc", "api.hip")
    assert '"eig_wide_form"' in _read("include", "romtime_hip.h")


def test_library_version_and_limit_without_a_gpu():
    """rt_version tells a host that the eigensolver entry points take n <= 2048."""
    from romtime_amd import _lib

    assert _lib.load().rt_version() >= 350
