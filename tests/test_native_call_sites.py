"""Structure of the package's native call sites (no GPU): each scan, statistics and
emission entry of libpmg_hip.so is called from one place, so a change of its argument
list is one edit (the signatures are untyped void pointers: a slip in a copy would be a
wild pointer on the device, not a TypeError)."""
import ast
import glob
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "poor_man_gplvm_amd")

ONE_SITE = (
    "pmg_forward_filter_phase", "pmg_forward_filter_batched",
    "pmg_backward_smoother_phase", "pmg_backward_smoother_batched",
    "pmg_dense_forward_phase", "pmg_dense_backward_phase",
    "pmg_suffstats", "pmg_suffstats_bf16", "pmg_suffstats_bf16x3",
    "pmg_emission_poisson", "pmg_emission_poisson_f64",
    "pmg_emission_rowref", "pmg_emission_rowref_batched",
)
# the engines reach the dense scans through the _phase entries (phase 3 = these)
NO_SITE = ("pmg_dense_forward", "pmg_dense_backward")


def _trees():
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 5, files
    for f in files:
        with open(f) as fh:
            yield os.path.basename(f), ast.parse(fh.read(), f)


def _callee_sites():
    """{attribute name: [file:line of every call expression whose callee is that attribute]}."""
    sites = {}
    for name, tree in _trees():
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
                sites.setdefault(node.func.attr, []).append(f"{name}:{node.lineno}")
    return sites


def test_one_call_site_per_native_entry():
    sites = _callee_sites()
    for entry in ONE_SITE:
        assert len(sites.get(entry, [])) <= 1, (entry, sites[entry])
    for entry in NO_SITE:
        assert not sites.get(entry), (entry, sites[entry])
    # the walk does see the call sites (the entries above are in use, not gone)
    assert sum(len(sites.get(entry, [])) for entry in ONE_SITE) == len(ONE_SITE)


def test_engine_classes_borrow_no_members():
    """No class body in engine.py assigns an attribute of another class
    (Name = OtherClass.attr): shared members live in a base class."""
    tree = dict(_trees())["engine.py"]
    classes = {n.name for n in ast.walk(tree) if isinstance(n, ast.ClassDef)}
    assert {"EngineBase", "DeviceEM", "RestartBatchEM"} <= classes
    for cls in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)):
        for stmt in cls.body:
            value = getattr(stmt, "value", None) if isinstance(stmt, (ast.Assign, ast.AnnAssign)) else None
            if isinstance(value, ast.Attribute) and isinstance(value.value, ast.Name):
                assert value.value.id not in classes, f"{cls.name} line {stmt.lineno}: borrows {value.value.id}.{value.attr}"
