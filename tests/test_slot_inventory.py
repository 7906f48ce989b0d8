"""Every attribute of the resident codecs' slots (`codec._Slot`, and the `codec._DecodeLane` and `codec._DecodeSlot` that
`BatchDecoder`, `BatchDecoder(coding_tile=...)` and `RegionDecoder` share) is classified in tests/slot_buffers.py: what a step may
find in it when it starts. tests/test_gpu_codec_slots.py poisons the SCRATCH ones between the steps of `BatchCodec` and
`BatchDecoder`, tests/test_gpu_region_decoder.py between those of `RegionDecoder`; a buffer added to a slot without a word here
would simply never be poisoned. CPU-only: it reads source text."""
import ast
import os

import slot_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODEC = os.path.join(ROOT, 'autoencoder_based_image_compression_amd', 'codec.py')


def _source():
    with open(CODEC) as f:
        return f.read()


def _lineage(tree, class_name):
    """The class's node and, behind it, those of its base classes defined in the same source, depth first in the order it names them
    (which is the order Python looks `__init__` up in for the single and the mixin-in-front inheritance codec.py uses)."""
    classes = {node.name: node for node in tree.body if isinstance(node, ast.ClassDef)}
    if class_name not in classes:
        raise AssertionError('codec.py has no class {0}'.format(class_name))
    (order, stack) = ([], [class_name])
    while stack:
        node = classes[stack.pop(0)]
        if node not in order:
            order.append(node)
            stack = [base.id for base in node.bases if isinstance(base, ast.Name) and base.id in classes] + stack
    return order


def _own_init(node):
    for item in node.body:
        if isinstance(item, ast.FunctionDef) and item.name == '__init__':
            return item
    return None


def _init_of(tree, class_name):
    """(the class, the `__init__` an instance of it runs first: its own, else the first one along its bases)."""
    lineage = _lineage(tree, class_name)
    for node in lineage:
        if _own_init(node) is not None:
            return lineage[0], _own_init(node)
    raise AssertionError('codec.py has no {0}.__init__'.format(class_name))


def _self_targets(target):
    """Names X of every `self.X` a (possibly nested tuple) assignment target holds."""
    if isinstance(target, (ast.Tuple, ast.List)):
        return [name for element in target.elts for name in _self_targets(element)]
    if isinstance(target, ast.Starred):
        return _self_targets(target.value)
    if isinstance(target, ast.Attribute) and isinstance(target.value, ast.Name) and target.value.id == 'self':
        return [target.attr]
    return []


def assigned_attributes(source, class_name):
    """Every attribute an instance of the class has: what its `__init__` and those of its base classes in the same source assign (in
    any branch), and every name of their `__slots__`."""
    names = set()
    for node in _lineage(ast.parse(source), class_name):
        init = _own_init(node)
        for sub in (ast.walk(init) if init is not None else ()):
            if isinstance(sub, ast.Assign):
                for target in sub.targets:
                    names.update(_self_targets(target))
            elif isinstance(sub, (ast.AugAssign, ast.AnnAssign)):
                names.update(_self_targets(sub.target))
        for item in node.body:
            if isinstance(item, ast.Assign) and any(isinstance(t, ast.Name) and t.id == '__slots__' for t in item.targets):
                names.update(ast.literal_eval(item.value))
    return names


def unclassified(source):
    """{class: sorted attributes its `__init__` assigns (or its `__slots__` names) that its table does not classify}."""
    out = {}
    for (class_name, table) in slot_buffers.TABLES.items():
        known = {slot_buffers.attribute_of(name) for name in table}
        out[class_name] = sorted(assigned_attributes(source, class_name) - known)
    return out


def _with_one_more_buffer(source, class_name):
    """`source` with `self.extra = torch.empty(...)` behind the last statement of the class's `__init__` (`_init_of`: its own, or the
    one it inherits first)."""
    (_, init) = _init_of(ast.parse(source), class_name)
    last = init.body[-1]
    lines = source.split('\n')
    lines.insert(last.end_lineno, ' '*last.col_offset + 'self.extra = torch.empty(16, dtype=torch.uint8, device=device)')
    return '\n'.join(lines)


def test_the_three_inits_parse():
    source = _source()
    slot = assigned_attributes(source, '_Slot')
    assert {'block', 'symbols', 'coder_streams', 'workspace', 'offsets', 'payload', 'staging', 'graphs', 'emit_host'} <= slot
    assert {'results', 'hist', 'overflow', 'flags', 'checks'} <= slot                  # a tuple target
    assert {'gathered', 'classes'} <= slot                                              # assigned as a pair
    assert {'head', 'head_bits', 'status', 'decoded', 'classes', 'scratch', 'unfinished', 'stream', 'placement', 'crop_origin'} <= \
        assigned_attributes(source, '_DecodeLane')
    assert {'lane', 'pinned_head', 'head_host', 'payload_host', 'planes', 'graph', 'count', 'crops'} <= assigned_attributes(source, '_DecodeSlot')


def test_every_assigned_attribute_is_classified():
    missing = {k: v for (k, v) in unclassified(_source()).items() if v}
    assert not missing, 'attributes of a slot that tests/slot_buffers.py does not classify (a buffer nobody poisons): {}'.format(missing)


def test_every_entry_exists_and_says_why():
    source = _source()
    for (class_name, table) in slot_buffers.TABLES.items():
        assigned = assigned_attributes(source, class_name)
        for (name, entry) in table.items():
            assert slot_buffers.attribute_of(name) in assigned, (class_name, name, 'is classified but no longer assigned')
            assert entry.cls in slot_buffers.CLASSES, (class_name, name)
            assert entry.reason.strip() and any(c.isdigit() for c in entry.reason), (class_name, name, 'needs a reason that names a line')
            if entry.cls == slot_buffers.CONTAINER:
                assert entry.parts and all(part in table and table[part].cls != slot_buffers.CONTAINER for part in entry.parts), (class_name, name)
            else:
                assert entry.parts is None, (class_name, name)
            if entry.alias is not None:
                assert entry.alias in table and table[entry.alias].cls == entry.cls and table[entry.alias].alias is None, (class_name, name)


def test_what_must_be_scratch_is_scratch():
    assert set(slot_buffers.MUST_BE_SCRATCH) == set(slot_buffers.TABLES)
    for (class_name, names) in slot_buffers.MUST_BE_SCRATCH.items():
        table = slot_buffers.TABLES[class_name]
        for name in names:
            assert name in table and table[name].cls == slot_buffers.SCRATCH, (class_name, name)
            assert table[name].alias is None, (class_name, name, 'must be poisoned itself')
    # the accumulators, counters and constants a step relies on are NOT scratch: poisoning them would hang a worker or derail a launch
    for (class_name, name) in (('_Slot', 'conv_ws'), ('_Slot', 'seq_dev'), ('_Slot', 'pinned_seq'), ('_Slot', 'hist'), ('_Slot', 'flags'),
                               ('_Slot', 'sse'), ('_Slot', 'table[:nb_maps]'), ('_DecodeLane', 'head_bytes'), ('_DecodeSlot', 'seq_dev'),
                               ('_DecodeSlot', 'pinned_seq')):
        assert slot_buffers.TABLES[class_name][name].cls in (slot_buffers.CARRIED, slot_buffers.CONSTANT), (class_name, name)


def test_an_unclassified_buffer_is_noticed():
    """The check has teeth: one more `self.extra = torch.empty(...)` in any of the three `__init__` bodies is reported, there only."""
    source = _source()
    for class_name in slot_buffers.TABLES:
        grown = _with_one_more_buffer(source, class_name)
        assert grown != source and 'extra' in assigned_attributes(grown, class_name)
        assert unclassified(grown) == {k: (['extra'] if k == class_name else []) for k in slot_buffers.TABLES}, class_name


# ---- the slot family of the rate-control codecs (tests/ratecontrol_slot_buffers.py) ------------------------------------------------

FAMILY = ('_BudgetSlot', '_TiledBudgetSlot', '_QualitySlot', '_TiledQualitySlot')


def _family_tables():
    import ratecontrol_slot_buffers
    return {'_BudgetSlot': ratecontrol_slot_buffers.slot_table(False, False), '_TiledBudgetSlot': ratecontrol_slot_buffers.slot_table(True, False),
            '_QualitySlot': ratecontrol_slot_buffers.slot_table(False, True), '_TiledQualitySlot': ratecontrol_slot_buffers.slot_table(True, True)}


def test_an_extra_buffer_of_a_family_member_shows_in_it_and_in_its_subclasses_only():
    """The four slot classes are a hierarchy: one more buffer in an `__init__` is unclassified in every class whose instances run
    that `__init__`, and nowhere else."""
    source = _source()
    tables = _family_tables()
    for (grown_class, shows_in) in (('_BudgetSlot', FAMILY), ('_QualitySlot', ('_QualitySlot', '_TiledQualitySlot')),
                                    ('_TiledRows', ('_TiledBudgetSlot', '_TiledQualitySlot')),
                                    # (the two tiled classes have no `__init__` of their own: the mixin in front of their bases has it)
                                    ('_TiledBudgetSlot', ('_TiledBudgetSlot', '_TiledQualitySlot')),
                                    ('_TiledQualitySlot', ('_TiledBudgetSlot', '_TiledQualitySlot'))):
        grown = _with_one_more_buffer(source, grown_class)
        assert grown != source
        for (class_name, table) in tables.items():
            known = {slot_buffers.attribute_of(name) for name in table}
            assert sorted(assigned_attributes(grown, class_name) - known) == (['extra'] if class_name in shows_in else []), (grown_class, class_name)
            assert sorted(assigned_attributes(source, class_name) - known) == [], class_name
        # and `_Slot` and the decoders' slots know nothing of it
        assert unclassified(grown) == {k: [] for k in slot_buffers.TABLES}


def test_no_family_member_lists_an_inherited_attribute_again():
    """`__slots__` of a class names what that class adds: no name stands in the `__slots__` of two classes of one lineage. (The two
    tiled classes are siblings and both add `class_rows`: Python does not combine two bases that both add slots.)"""
    tree = ast.parse(_source())
    for class_name in FAMILY:
        seen = []
        for node in _lineage(tree, class_name):
            for item in node.body:
                if isinstance(item, ast.Assign) and any(isinstance(t, ast.Name) and t.id == '__slots__' for t in item.targets):
                    seen.extend(ast.literal_eval(item.value))
        assert len(seen) == len(set(seen)), (class_name, sorted(name for name in set(seen) if seen.count(name) > 1))
