"""What every buffer of the rate-control codecs' per-step state may hold when a step starts: tests/slot_buffers.py's classification
for what a step of `codec.BudgetCodec`, `TiledBudgetCodec`, `QualityCodec` and `TiledQualityCodec` owns beyond its `_Slot` (a plain
helper module: import it, no fixture lives here). The four slot classes are one family (`_BudgetSlot`, `_TiledRows` in front of it,
`_QualitySlot` behind it), and so are their tables: `slot_table(tiled, quality)` builds one from the budget entries, a tiled
overlay (`class_rows`, the rows per stream, the kernels' names) and a quality overlay (the search's entries; `point` becomes `first`).
tests/budget_slot_buffers.py, tiled_budget_slot_buffers.py, quality_slot_buffers.py and tiled_quality_slot_buffers.py give them their
names; the four `test_*_host.py` beside them keep them complete, the GPU tests poison the SCRATCH entries between steps.

The reasons name the function of codec.py, device.py or the kernel of csrc/hip the entry rests on, and the step of the launch table of
the variant's own section of DESIGN.md (19 to 22) it is defined in: for every SCRATCH entry the launch (or host write) of the SAME
step that defines it in front of its first reader."""
import torch

import slot_buffers
from slot_buffers import CONSTANT, CONTAINER, NOT_A_BUFFER, SCRATCH, _entry

# the number every launch has in the launch table of DESIGN.md section 19, 20, and 21 = 22
_STEPS = {
    (False, False): dict(section=19, zero=1, ladder=4, fetch=5, select=6, quantiser=7, exception=8, coder=9, publish=11),
    (True, False): dict(section=20, zero=1, ladder=3, fetch=4, select=5, quantiser=6, exception=8, coder=10, publish=13),
    (False, True): dict(section=21, zero=1, ladder=3, fetch=4, select=5, fetch_sse=6, round_0=7, probe=8, round=9, quantiser=10,
                        exception=11, coder=12, publish=14),
    (True, True): dict(section=22, zero=1, ladder=3, fetch=4, select=5, fetch_sse=6, round_0=7, probe=8, round=9, quantiser=10,
                       exception=11, coder=12, publish=14),
}


def slot_table(tiled, quality):
    """{attribute: Entry} of `_BudgetSlot` (neither), `_TiledBudgetSlot` (tiled), `_QualitySlot` (quality) or `_TiledQualitySlot`."""
    s = _STEPS[(tiled, quality)]
    tiles = '_tiles' if tiled else ''
    (ladder, select, search) = ('ladder{0}_kernel'.format(tiles), 'ladder_select{0}_kernel'.format(tiles), 'quality_search{0}_kernel'.format(tiles))
    (codec, worker) = ('`QualityCodec', '`_QualityWorker._finish`') if quality else ('`BudgetCodec', '`_BudgetWorker._finish`')
    point = 'first' if quality else 'point'          # the block `ladder_select` writes every image's point into
    streams = ' of N x K x T x 128 streams' if tiled else ''
    zeroed = ('step {zero}: `accum.zero_()` is the first launch of `BudgetCodec._launch_selection` and covers all of `accum`; step {ladder}: '
              '{0} then adds into it (ladder.hip), in front of {1}, its only reader (step {select})').format(ladder, select, **s)
    if quality:
        selected = ('step {select}: {0} writes every element on every call (budget.hip; `_launch_select` hands it `first`, the slot\'s '
                    '`selected`, as its point) in front of its readers: {1} (steps {round_0}, {round}) and the publication (step '
                    '{publish})').format(select, search, **s)
    else:
        selected = ('step {select}: {0} writes every element on every call (budget.hip: point and flags by thread 0, upper by the first K '
                    'threads of every image\'s block) in front of its readers: latent_rows_kernel (step {quantiser}), the coder (step {coder}) '
                    'and the publication (step {publish})').format(select, **s)
    # who writes the coder's rows, and who names no exception row where there is no exception map
    if tiled:
        rows = 'step {select}: tile_prob_rows_kernel, the second launch of eae_hip_ladder_select_tiles, writes all n_streams = entries x 128 rows'
        rows_writer = search if quality else 'tile_prob_rows_kernel'
    else:
        rows = 'step {select}: ladder_select_kernel writes all N x 128 rows'
        rows_writer = search if quality else 'ladder_select_kernel'
    if quality:
        rows += (' (budget.hip), and so does every round of {0} (steps {round_0}, {round}' + (': `run_entry` is a permutation of the entries, '
                 'each image\'s block writes its own T' if tiled else '') + '), the last one in front of the coder (step {coder})')
    else:
        rows += ' (budget.hip) in front of the coder (step {coder})'
    table = {
        'accum': _entry(CONTAINER, '`_BudgetSlot.__init__`, step {zero}: [bypass bits | histograms | range errors]{0}, zeroed as one'
                        .format(streams, **s), parts=('bypass_bits', 'hist', 'range_errors')),
        'bypass_bits': _entry(SCRATCH, zeroed),
        'hist': _entry(SCRATCH, zeroed),
        'range_errors': _entry(SCRATCH, zeroed + '; nothing reads it: a point with range errors shows as an incomplete histogram (s_count, '
                                                 'budget.hip)'),
        'pinned_budgets': _entry(SCRATCH, '{0}._stage` writes the batch_size budgets of the step before its first launch{1}; the pad word of an '
                                          'odd batch is copied and never read (step {select} passes budgets[:batch_size])'
                                 .format(codec, ' (2^62 without a budget)' if quality else '', **s)),
        'budgets_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_budgets, which `_stage` writes through it (step 0)'),
        'budgets': _entry(SCRATCH, 'step {fetch}: fetch_prefix copies budgets_nbytes = ALL of pinned_budgets in front of {0} (step {select})'
                          .format(select, **s)),
        'budgets_nbytes': _entry(CONSTANT, 'the size of the budget block (8 bytes per image, padded to 16), written at construction, read by '
                                           'fetch_prefix'),
        'select': _entry(CONTAINER, '`_BudgetSlot.__init__`, step {publish}: [upper | {0} | flags], published as one'.format(point, **s),
                         parts=('upper', point, 'flags')),
        'upper': _entry(SCRATCH, selected),
        point: _entry(SCRATCH, selected),
        'flags': _entry(SCRATCH, selected),
        'prob_row': _entry(SCRATCH, rows.format(search, **s)),
        'pinned_select': _entry(SCRATCH, 'step {publish}: publish_to_host copies all of `select` in front of the coder side\'s step counter '
                                         '(`BudgetCodec._publish_coder_side`)'.format(**s)),
        'select_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select, filled in step {publish}: upper, {0}, flags'.format(point, **s)),
        'table': _entry(CONTAINER, '`_BudgetSlot.__init__`, step {coder}: [the K x 128 rows of the ladder | one row per image]'.format(**s),
                        parts=('points_table', 'exception_rows')),
        'points_table': _entry(CONSTANT, 'the ladder\'s K x 128 probability rows, copied at construction and only read by the coder'),
        'exception_rows': _entry(SCRATCH, 'step {exception}: with an exception map exception_rows_kernel writes all L entries of every image\'s '
                                          'row in front of the coder (codec_container.hip); without one no prob_row names them ({0}: '
                                          'idx_exception = -1 matches no map) and the worker takes none ({1})'.format(rows_writer, worker, **s)),
        'pinned_rows': _entry(SCRATCH, 'step {publish}: with an exception map publish_to_host copies all of exception_rows in front of the step '
                                       'counter; without one the worker does not read it ({0}: idx_map_exception < 0)'.format(worker, **s)),
        'rows_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_rows, filled in step {publish}'.format(**s)),
    }
    if tiled:
        table['class_rows'] = _entry(SCRATCH, 'views of `prob_row`, one per shape class (`_TiledRows.__init__`: `coding_tile_layout`\'s runs '
                                              'cover all n_streams)', alias='prob_row')
    if quality:
        round_0 = ('step {round_0}: round 0 of {0} writes every element of every output (quality.hip: search_round, thread 0 of every '
                   'image\'s block) in front of the first probe (step {probe}); ').format(search, **s)
        table['select'] = _entry(CONTAINER, '`_BudgetSlot.__init__` with `_QualitySlot`\'s extra words, step {publish}: [upper | first | flags | '
                                            'trace_sse | point | met | state | trace_point], published as one'.format(**s),
                                 parts=('upper', 'first', 'flags', 'trace_sse', 'point', 'met', 'state', 'trace_point'))
        table.update({
            'pinned_max_sse': _entry(SCRATCH, '`QualityCodec._stage` writes the batch_size thresholds of the step before its first launch; the '
                                              'pad word of an odd batch is copied and never read (`_launch_round` passes max_sse[:batch_size])'),
            'max_sse_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_max_sse, which `_stage` writes through it (step 0)'),
            'max_sse': _entry(SCRATCH, 'step {fetch_sse}: fetch_prefix copies max_sse_nbytes = ALL of pinned_max_sse in front of round 1 of {0}, '
                                       'its first reader (step {round}; round 0 does not read it)'.format(search, **s)),
            'max_sse_nbytes': _entry(CONSTANT, 'the size of the threshold block (8 bytes per image, padded to 16), written at construction, read '
                                               'by fetch_prefix'),
            'trace_sse': _entry(SCRATCH, round_0 + '-1 everywhere, then round r writes column r - 1 (step {round})'.format(**s)),
            'trace_point': _entry(SCRATCH, round_0 + '-1 everywhere, then round r writes column r - 1 (step {round})'.format(**s)),
            'point': _entry(SCRATCH, round_0 + 'every round writes it again in front of the quantiser that reads it (steps {probe}, {quantiser})'
                            .format(**s)),
            'met': _entry(SCRATCH, round_0 + 'every round writes it again, the last one the answer'),
            'state': _entry(SCRATCH, round_0 + 'round r >= 1 reads what round r - 1 of the same step wrote'),
            'search_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select, filled in step {publish}: point, met, trace_point, trace_sse'.format(**s)),
            'probe_acc': _entry(SCRATCH, round_0 + '0; tconv3_kernel of a probe adds the squared errors (step {probe}), the round behind it reads '
                                                   'and zeroes them (step {round})'.format(**s)),
            'probe_latent': _entry(SCRATCH, 'step {probe}: latent_rows_kernel writes every latent of every image (t_out, or shifted_out of the '
                                            'learned model) in front of the probe\'s tconv1, its only reader'.format(**s)),
        })
    return table


def must_be_scratch(quality):
    """The entries the GPU tests rely on being poisoned, whatever the table says of the others."""
    names = ('bypass_bits', 'hist', 'range_errors', 'pinned_budgets', 'budgets', 'upper', 'first' if quality else 'point', 'flags', 'prob_row',
             'pinned_select', 'exception_rows', 'pinned_rows')
    if quality:
        names += ('pinned_max_sse', 'max_sse', 'trace_sse', 'trace_point', 'point', 'met', 'state', 'probe_acc', 'probe_latent')
    return names


def slots_of(codec):
    """The per-step state beyond `_Slot` of every slot of a rate-control codec, in the slots' order."""
    return [codec._budget_slots[id(slot)] for slot in codec._slots]


def poison_scratch(codec, table, byte):
    """Fills every SCRATCH buffer `table` names of every one of `slots_of(codec)`, device and pinned alike (aliases such as
    `class_rows` through what they view; `slot_buffers.poison_scratch` does the `_Slot`s). The codec must be idle. Returns the number
    of bytes filled."""
    total = 0
    for owner in slots_of(codec):
        for (_, tensor) in slot_buffers.scratch_leaves(owner, table):
            slot_buffers.fill_bytes(tensor, byte)
            total += tensor.numel()*tensor.element_size()
    torch.cuda.synchronize()
    return total


def check_entries(table, assigned, scratch, constants, needs_digit=False):
    """Every entry of `table` is one of `assigned` (the attributes the slot class has), has a class and says why (needs_digit: names
    a line or a step); a CONTAINER names classified parts that are none themselves, and nothing else has parts; `class_rows` is the
    one alias; `scratch` are SCRATCH and `constants` CONSTANT."""
    for (name, entry) in table.items():
        assert slot_buffers.attribute_of(name) in assigned, (name, 'is classified but no longer assigned')
        assert entry.cls in slot_buffers.CLASSES, name
        assert entry.reason.strip(), name
        if needs_digit:
            assert any(c.isdigit() for c in entry.reason), (name, 'needs a reason that names a line')
        if entry.cls == CONTAINER:
            assert entry.parts and all(part in table and table[part].cls != CONTAINER for part in entry.parts), name
        else:
            assert entry.parts is None, name
        assert (entry.alias is None) == (name != 'class_rows'), name
    for name in scratch:
        assert table[name].cls == SCRATCH, name
    for name in constants:
        assert table[name].cls == CONSTANT, name
