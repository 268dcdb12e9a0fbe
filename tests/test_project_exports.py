"""The resident projection is declared in every layer: header, export list, Python handle and group (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nl_stack_frame_project_from", "nl_group_frame_project_from")


def test_header_declares_the_resident_projection():
    with open(os.path.join(ROOT, "include", "nlstack.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_exports_and_python_methods():
    from nightlight_amd import capi
    from nightlight_amd.stack import StackGroup, StackHandle
    for name in NAMES:
        assert name in capi.EXPORTS
    assert callable(getattr(StackHandle, "frame_project_from", None))
    assert callable(getattr(StackGroup, "frame_project_from", None))
