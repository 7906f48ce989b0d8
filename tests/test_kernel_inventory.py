"""Every entry point of include/eae_hip.h is exercised by some GPU test: named in a tests/test_gpu_*.py module (or another
module marked `gpu` as a whole) either directly (`eae_hip_*`) or through the device.py wrapper that calls it. A new kernel
without a test turns this red; so does removing the only test module that covers one. CPU-only: it reads source text."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'eae_hip.h')
DEVICE = os.path.join(ROOT, 'autoencoder_based_image_compression_amd', 'device.py')

# Entry points no GPU test module has to name, each with the reason.
ALLOWED_UNTESTED = {
    'eae_hip_version': 'a version string, checked by tests/test_abi.py',
    'eae_hip_device_info': 'reports the device; no result to compare',
    'eae_hip_debug_set_stamp_buffer': 'test build only: a profiling hook that records timestamps, no result to compare',
    'eae_hip_debug_reload_launch_options': 'test build only: called by the launch_options fixture of tests/conftest.py',
    'eae_hip_coder_trailing_workspace_bytes': 'experimental build only: sizes the workspace coder_roundtrip_trailing / _fused '
                                              'allocate themselves when tests/test_coder_device.py runs them',
}


def _strip_comments(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', text)


def declared_functions():
    """Names of the functions the header declares (comments removed; typedefs and macros have no parameter list)."""
    with open(HEADER) as f:
        text = _strip_comments(f.read())
    return sorted(set(re.findall(r'\b(eae_hip_\w+)\s*\(', text)))


def wrappers():
    """eae_hip_* name -> names of the device.py functions (and classes, for their methods) whose body calls it."""
    with open(DEVICE) as f:
        tree = ast.parse(f.read())
    found = {}

    def visit(node, names):
        for sub in ast.walk(node):
            if isinstance(sub, ast.Attribute) and sub.attr.startswith('eae_hip_'):
                found.setdefault(sub.attr, set()).update(names)

    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            visit(node, {node.name})
        elif isinstance(node, ast.ClassDef):
            for item in node.body:
                if isinstance(item, ast.FunctionDef):
                    names = {node.name} if item.name.startswith('__') else {node.name, item.name}
                    visit(item, names)
    return found


def gpu_test_texts():
    """The GPU test modules: tests/test_gpu_*.py and any other module marked `gpu` as a whole (test_coder_device.py)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'test_*.py'))):
        with open(path) as f:
            text = f.read()
        if os.path.basename(path).startswith('test_gpu_') or re.search(r'^pytestmark = pytest\.mark\.gpu$', text, flags=re.M):
            out[os.path.basename(path)] = text
    return out


def _named(text, name):
    """`name` appears as a call or an attribute (dev.name / name(...)), not as part of a longer identifier."""
    return re.search(r'(?<![\w])' + re.escape(name) + r'(?![\w])\s*\(|\.' + re.escape(name) + r'(?![\w])', text) is not None


def coverage(texts=None):
    texts = gpu_test_texts() if texts is None else texts
    wrap = wrappers()
    out = {}
    for function in declared_functions():
        names = {function} | wrap.get(function, set())
        out[function] = sorted(module for (module, text) in texts.items() if any(_named(text, name) for name in names))
    return out


def test_header_parses():
    functions = declared_functions()
    assert len(functions) > 50
    for expected in ('eae_hip_svhn_dense_f64', 'eae_hip_map_minmax', 'eae_hip_cast_int16', 'eae_hip_dequantize_maps',
                     'eae_hip_coder_pack_streams', 'eae_hip_tile_copy', 'eae_hip_debug_check_mid_forms'):
        assert expected in functions
    wrap = wrappers()
    assert wrap['eae_hip_svhn_dense_f64'] == {'svhn_dense'}
    assert 'Model' in wrap['eae_hip_model_create']


def test_every_entry_point_is_named_by_a_gpu_test():
    cov = coverage()
    missing = sorted(f for (f, modules) in cov.items() if not modules and f not in ALLOWED_UNTESTED)
    assert not missing, 'entry points of include/eae_hip.h that no tests/test_gpu_*.py names (directly or through ' \
                        'their device.py wrapper): {}'.format(missing)


def test_allow_list_is_current():
    functions = set(declared_functions())
    assert set(ALLOWED_UNTESTED) <= functions, sorted(set(ALLOWED_UNTESTED) - functions)
    assert all(reason.strip() for reason in ALLOWED_UNTESTED.values())


def test_removing_a_module_is_noticed():
    """The check has teeth: without the modules that test the small kernels directly, some entry point is uncovered. (The
    buffer-discipline module reruns every kernel between guard bands with the helpers it imports from these modules, so it leaves
    with them.)"""
    texts = gpu_test_texts()
    for module in ('test_gpu_svhn_kernels.py', 'test_gpu_quantize_helpers.py'):
        assert module in texts and 'test_gpu_buffer_discipline.py' in texts
        rest = {k: v for (k, v) in texts.items() if k not in (module, 'test_gpu_buffer_discipline.py')}
        lost = sorted(f for (f, modules) in coverage(rest).items() if modules == [] and f not in ALLOWED_UNTESTED)
        assert lost, module
