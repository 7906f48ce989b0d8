"""What `codec.TiledQualityCodec` rests on, on the host: `codec.tile_prob_rows`, the rows
`device.quality_search_tiles` must write, against the layout's own rows and `container._prob_rows` per class; the inventory of
`codec._TiledQualitySlot` against tests/tiled_quality_slot_buffers.py; the signature of `container.encode_images_to_quality`. CPU only,
numpy only."""
import inspect
import os

import numpy

import ratecontrol_slot_buffers
import slot_buffers
import tiled_quality_slot_buffers
from test_slot_inventory import _with_one_more_buffer, assigned_attributes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODEC = os.path.join(ROOT, 'autoencoder_based_image_compression_amd', 'codec.py')
NB_MAPS = 128
# (images, latent plane, coding tile) -> (tiles of an image, shape classes)
LAYOUTS = [((3, 11, 13, (4, 4)), 12, 4), ((3, 11, 13, (16, 16)), 1, 1), ((5, 8, 8, (4, 4)), 4, 1), ((1, 11, 13, (4, 4)), 12, 4), ((2, 3, 7, (2, 3)), 6, 4)]


def test_the_rows_are_the_layouts_own_when_every_point_is_zero():
    from autoencoder_based_image_compression_amd import codec
    for ((n, h, w, tile), nb_tiles, nb_classes) in LAYOUTS:
        for exception in (-1, 0, 5, 127):
            layout = codec.coding_tile_layout(n, h, w, tile, exception)
            assert (layout['nb_tiles'], len(layout['runs'])) == (nb_tiles, nb_classes)
            rows = codec.tile_prob_rows(layout, numpy.zeros(n, dtype=numpy.int64), exception)
            assert rows.dtype == numpy.int32 and rows.shape == (layout['n_streams'],)
            assert numpy.array_equal(rows, layout['prob_row'])
            assert numpy.array_equal(codec.tile_prob_rows(layout, [0]*n, exception, NB_MAPS), layout['prob_row'])


def test_the_rows_in_run_order_stated_entry_by_entry():
    """Run-order entry e is the (image, tile) `payload_entry[e]` names: its map m takes points[image]*128 + m, its exception map
    exception_row_base + image; class by class these are `container._prob_rows` moved to the image's point."""
    from autoencoder_based_image_compression_amd import codec, container
    rng = numpy.random.RandomState(3)
    for ((n, h, w, tile), nb_tiles, _) in LAYOUTS:
        for (k_points, exception) in ((1, -1), (3, 5), (9, 5), (9, -1)):
            layout = codec.coding_tile_layout(n, h, w, tile, exception)
            points = rng.randint(0, k_points, size=n)
            base = k_points*NB_MAPS
            rows = codec.tile_prob_rows(layout, points, exception, base).reshape(n*nb_tiles, NB_MAPS)
            for e in range(n*nb_tiles):
                (image, tile_index) = layout['entries'][int(layout['payload_entry'][e])]
                assert int(layout['run_entry'][image*nb_tiles + tile_index]) == e
                expected = int(points[image])*NB_MAPS + numpy.arange(NB_MAPS)
                if exception >= 0:
                    expected[exception] = base + image
                assert numpy.array_equal(rows[e], expected), (e, image)
            # per shape class: `container._prob_rows` names rows m and 128 + image; moved to the image's point and the codec's base
            first = 0
            for (_, count, first_stream, _) in layout['runs']:
                ks = layout['payload_entry'][first:first + count].tolist()
                plain = container._prob_rows(layout['entries'], ks, exception).reshape(count, NB_MAPS).astype(numpy.int64)
                images = numpy.array([layout['entries'][k][0] for k in ks])
                moved = plain + points[images][:, None]*NB_MAPS
                if exception >= 0:
                    moved[:, exception] = plain[:, exception] - NB_MAPS + base
                assert first_stream == first*NB_MAPS and numpy.array_equal(rows[first:first + count], moved)
                first += count
            assert first == n*nb_tiles
            if exception >= 0:
                # the default base lies behind the rows of the finest K points that hold every point named
                assert numpy.array_equal(codec.tile_prob_rows(layout, points, exception), codec.tile_prob_rows(layout, points, exception,
                                                                                                                (int(points.max()) + 1)*NB_MAPS))


# ---- the inventory of codec._TiledQualitySlot ------------------------------------------------------------------------------------

def _source():
    with open(CODEC) as f:
        return f.read()


def _unclassified(source):
    known = {slot_buffers.attribute_of(name) for name in tiled_quality_slot_buffers.TILED_QUALITY_SLOT}
    return sorted(assigned_attributes(source, '_TiledQualitySlot') - known)


def test_every_attribute_of_the_tiled_quality_slot_is_classified():
    assigned = assigned_attributes(_source(), '_TiledQualitySlot')
    assert {'accum', 'select', 'first', 'point', 'met', 'state', 'trace_point', 'trace_sse', 'pinned_max_sse', 'max_sse', 'probe_acc',
            'probe_latent', 'prob_row', 'class_rows', 'table'} <= assigned
    assert _unclassified(_source()) == []
    # `_QualitySlot`'s state and `_TiledBudgetSlot`'s rows per class, nothing else
    assert assigned == assigned_attributes(_source(), '_QualitySlot') | {'class_rows'}


def test_every_entry_of_the_tiled_quality_slot_exists_and_says_why():
    table = tiled_quality_slot_buffers.TILED_QUALITY_SLOT
    ratecontrol_slot_buffers.check_entries(table, assigned_attributes(_source(), '_TiledQualitySlot'), tiled_quality_slot_buffers.MUST_BE_SCRATCH,
                                           ('budgets_nbytes', 'max_sse_nbytes', 'points_table'))
    assert table['class_rows'].alias == 'prob_row'
    assert not any(entry.cls == slot_buffers.CARRIED for entry in table.values())       # a step depends on nothing the last one left


def test_an_unclassified_buffer_of_the_tiled_quality_slot_is_noticed():
    assert _unclassified(_with_one_more_buffer(_source(), '_TiledQualitySlot')) == ['extra']


def test_the_other_slots_did_not_grow():
    """`_TiledQualitySlot` exists so that its siblings keep their attributes: their helpers still classify all of them."""
    import budget_slot_buffers
    import quality_slot_buffers
    import tiled_budget_slot_buffers
    for (name, table) in (('_Slot', slot_buffers.SLOT), ('_BudgetSlot', budget_slot_buffers.BUDGET_SLOT),
                          ('_TiledBudgetSlot', tiled_budget_slot_buffers.TILED_BUDGET_SLOT), ('_QualitySlot', quality_slot_buffers.QUALITY_SLOT)):
        assert assigned_attributes(_source(), name) <= {slot_buffers.attribute_of(key) for key in table}, name


# ---- the public signatures ----------------------------------------------------------------------------------------------------------

def test_the_host_loop_keeps_its_positional_order():
    from autoencoder_based_image_compression_amd import container
    parameters = inspect.signature(container.encode_images_to_quality).parameters
    assert list(parameters) == ['luminances_uint8', 'encoder', 'decoder', 'ladder', 'target_psnr', 'max_sse', 'budget_bytes', 'coding_tile']
    assert [parameters[name].default for name in ('target_psnr', 'max_sse', 'budget_bytes', 'coding_tile')] == [None]*4


def test_the_codec_takes_the_tile_where_its_siblings_do():
    from autoencoder_based_image_compression_amd import codec
    assert issubclass(codec.TiledQualityCodec, codec.QualityCodec) and codec.TiledQualityCodec._budget_slot_class is codec._TiledQualitySlot
    assert codec.TiledQualityCodec._worker_class is codec._QualityWorker
    assert codec.TiledQualityCodec._takes_coding_tile and not codec.QualityCodec._takes_coding_tile and not codec.BudgetCodec._takes_coding_tile
    parameters = list(inspect.signature(codec.TiledQualityCodec.__init__).parameters)
    assert parameters[:12] == ['self', 'variables', 'are_bin_widths_learned', 'ladder', 'batch_size', 'h_in', 'w_in', 'coding_tile', 'target_psnr',
                               'max_sse', 'budget_bytes', 'batch_codec_options']
