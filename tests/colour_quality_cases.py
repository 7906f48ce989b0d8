"""What tests/test_gpu_colour_quality_container.py and tests/test_gpu_colour_quality_codec.py share (a plain helper module: import it,
no fixture lives here): the reference table of squared errors, built without any code of DESIGN.md section 30, the numpy statement of
that section's rule on the table, and the thresholds both modules derive from the table.

The configurations, ladders and pictures are those of tests/colour_budget_cases.py. For every plane of every picture and every point
of the plane's ladder the table holds the squared error of `decode_images(encode_images(plane, ..., pad=True))` against the real
plane, summed in numpy: the container path that existed before the colour quality floor."""
import numpy

import colour_budget_cases as cases

TOP = 1 << 62
SHARES = (0.25, 1./3., 0.9)


class Case(object):
    """One configuration and batch: pictures, planes, ladders, the plane blobs at every point and the table, made once."""

    def __init__(self, models, config, seed=0):
        from autoencoder_based_image_compression_amd import colour, container
        (self.learned, _, self.nb_points, self.size, self.count, _, _) = cases.CONFIGS[config]
        (self.ladder, self.chroma_ladder) = cases.ladders_of(models, config)
        self.ladders = (self.ladder,) + (self.chroma_ladder or self.ladder,)*2
        (self.variables, self.encoder, self.decoder) = (models[self.learned][key] for key in ('variables', 'encoder', 'decoder'))
        self.rgb = cases.pictures(config, seed)
        self.planes = colour.split_420_numpy(self.rgb)
        self.blobs = {}
        self.table = numpy.zeros((self.count, 3, self.nb_points), dtype=numpy.int64)
        for (which, (plane, ladder)) in enumerate(zip(self.planes, self.ladders)):
            for i in range(self.count):
                for k in range(self.nb_points):
                    more = {} if ladder.rdo_lambdas is None else {'rdo_lambda': ladder.rdo_lambdas[k]}
                    blob = container.encode_images(plane[i:i + 1], self.encoder, ladder.bin_widths_points[k], ladder.map_mean,
                                                   ladder.binary_probabilities_points[k], ladder.idx_map_exception, pad=True, **more)[0]
                    decoded = container.decode_images(blob, self.decoder)
                    assert decoded.shape == plane[i:i + 1].shape
                    difference = plane[i:i + 1].astype(numpy.int64) - decoded.astype(numpy.int64)
                    self.blobs[(which, i, k)] = blob
                    self.table[i, which, k] = (difference*difference).sum()

    def picture_blob(self, i, points):
        from autoencoder_based_image_compression_amd import container
        return container.assemble_colour_blob(self.size, *(self.blobs[(which, i, int(points[which]))] for which in range(3)))

    def threshold_sets(self):
        """One int64 (N,) per step: 0; 2^62; for every k the sum of the three table entries at (k, k, k), and that sum less 1."""
        sets = [numpy.zeros(self.count, dtype=numpy.int64), numpy.full(self.count, TOP, dtype=numpy.int64)]
        for k in range(self.nb_points):
            exact = self.table[:, :, k].sum(axis=1)
            sets += [exact, exact - 1]
        return sets


def case_of(models, config, seed=0):
    key = ('colour_quality_case', config, seed)
    if key not in models:
        models[key] = Case(models, config, seed)
    return models[key]


def rule(table, thresholds, share):
    """The rule of DESIGN.md section 30 on a table sse int64 (N, 3, K) in the order Y, Cb, Cr, every search from point 0 -> a dict
    of what a step must report, with the functions of ratecontrol.py that existed before it (`select_by_quality`) and plain integers."""
    from autoencoder_based_image_compression_amd import ratecontrol
    (n, _, nb_points) = table.shape
    thresholds = numpy.broadcast_to(numpy.asarray(thresholds, dtype=numpy.int64), (n,))
    q16 = int(round(float(share)*65536))
    a = numpy.array([(int(m)*q16) >> 17 for m in thresholds.tolist()], dtype=numpy.int64)
    first = numpy.zeros(n, dtype=numpy.int64)
    (k_cb, met_cb, probes_cb, probed_cb) = ratecontrol.select_by_quality(table[:, 1], first, a)
    (k_cr, met_cr, probes_cr, probed_cr) = ratecontrol.select_by_quality(table[:, 2], first, a)
    rows = numpy.arange(n)
    rest = numpy.array([max(int(m) - int(b) - int(r), 0) for (m, b, r) in zip(thresholds.tolist(), table[rows, 1, k_cb].tolist(),
                                                                                table[rows, 2, k_cr].tolist())], dtype=numpy.int64)
    (k_y, met_y, probes_y, probed_y) = ratecontrol.select_by_quality(table[:, 0], first, rest)
    points = numpy.stack([k_y, k_cb, k_cr], axis=1)
    sse = numpy.stack([table[rows, which, points[:, which]] for which in range(3)], axis=1)
    return {'rate_point': points, 'met': numpy.stack([met_y, met_cb, met_cr], axis=1), 'max_sse': numpy.stack([rest, a, a], axis=1),
            'probe_points': numpy.stack([probes_y, probes_cb, probes_cr], axis=1), 'probe_sse': numpy.stack([probed_y, probed_cb, probed_cr], axis=1),
            'sse': sse, 'picture_sse': sse.sum(axis=1), 'picture_max_sse': thresholds.copy(), 'picture_met': sse.sum(axis=1) <= thresholds}


def assert_the_set_tells(table, sets, share):
    """ON THE REFERENCE'S outcome: over a configuration's threshold sets at least two luminance points occur and `picture_met` occurs
    both true and false. If the table does not give that, the inputs are wrong."""
    outcomes = [rule(table, thresholds, share) for thresholds in sets]
    assert len({int(k) for outcome in outcomes for k in outcome['rate_point'][:, 0]}) >= 2
    met = {bool(m) for outcome in outcomes for m in outcome['picture_met']}
    assert met == {False, True}
    return outcomes
