"""The layout of the test suite: test modules are leaves.  Shared code lives in the support modules of tests/ (names that do not start with
test_), so nothing imports a test module -- a test's outcome cannot depend on which other files were collected -- and no support module
holds a test.  Read from the sources with ast; nothing is imported but the table of stream cases."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sources(*dirs):
    for d in dirs:
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            if f.endswith('.py'):
                path = os.path.join(ROOT, d, f)
                with open(path) as fh:
                    yield os.path.join(d, f), ast.parse(fh.read(), path)


def imported_test_modules(tree):
    """every `tests.test_*` module a source imports, at any nesting depth: from tests import test_x / from tests.test_x import y /
    import tests.test_x (relative imports inside the package count as tests.*)"""
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            module = node.module or ''
            if node.level:
                module = 'tests.' + module if module else 'tests'
            if module == 'tests':
                found += ['tests.' + a.name for a in node.names if a.name.startswith('test_')]
            elif module.startswith('tests.test_'):
                found.append(module)
        elif isinstance(node, ast.Import):
            found += [a.name for a in node.names if a.name.startswith('tests.test_')]
    return found


def test_the_import_finder_sees_every_form():
    tree = ast.parse("from tests import helpers, test_a as a\nimport tests.test_b\nimport os\n"
                     "def f():\n    from tests.test_c import x\n    from . import test_d\n    from .test_e import y\n    from tests.helpers import z\n")
    assert imported_test_modules(tree) == ['tests.test_a', 'tests.test_b', 'tests.test_c', 'tests.test_d', 'tests.test_e']


def test_nothing_imports_a_test_module():
    bad = {path: mods for path, tree in _sources('tests', 'tools') for mods in [imported_test_modules(tree)] if mods}
    assert not bad, "test modules are leaves; move what is shared into a support module of tests/: %s" % bad


def test_support_modules_define_no_tests():
    bad = {path: names for path, tree in _sources('tests') if not os.path.basename(path).startswith('test_')
           for names in [[n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith('test_')]] if names}
    assert not bad, "functions named test_* in modules pytest does not collect: %s" % bad


def test_the_stream_cases_have_unique_ids():
    from tests.stream_cases import CASES
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids), "ids that stand twice in the table of stream cases: %s" % sorted({i for i in ids if ids.count(i) > 1})
