"""Times the neural operator entry points at any layer widths on configs[2]'s graph (5 000 x n = 200, m = 840: 12.6 M edges): the GRU cell,
the edge aggregator in both directions, the predictor, and one whole np-nd-np sweep (two aggregations, two GRU cells, one prediction), as ms per
launch and the fraction of the fp32 MFMA peak (157.3 TFLOP/s) the operator's multiply-adds make of it.  The defaults are the widths of the
reference config p-prodec2-modular-variable-pytorch-2.yaml (hidden 200, mem 150, agg 150, mem_agg 100, classifier 100).
Usage: python tools/wide_ops_time.py [--hidden H] [--mem M] [--agg G] [--mem-agg A] [--classifier C] [--n N] [--reps R]
PDP_NEURAL_GENERIC=1 runs the generic tile kernels where they take the shape (the comparison at hidden 190: Kpx = 192)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pdp-solver_amd'))
from pdp.factorgraph import dataset  # noqa: E402
from pdp import native  # noqa: E402

PEAK = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument('--hidden', type=int, default=200)
ap.add_argument('--mem', type=int, default=150)
ap.add_argument('--agg', type=int, default=150)
ap.add_argument('--mem-agg', dest='mem_agg', type=int, default=100)
ap.add_argument('--classifier', type=int, default=100)
ap.add_argument('--n', type=int, default=200)
ap.add_argument('--batch', type=int, default=5000)
ap.add_argument('--reps', type=int, default=5)
args = ap.parse_args()
H, m1, g, a, c = args.hidden, args.mem, args.agg, args.mem_agg, args.classifier

dev = torch.device('cuda:0')
tb = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(args.batch, args.n, 3, m=int(round(4.2 * args.n)), seed=0)), dev)
p = native.Problem(tb['graph_map'], tb['batch_variable_map'], tb['batch_function_map'], tb['edge_feature'])
E, V = p.E, p.V
gen = torch.Generator(device='cpu'); gen.manual_seed(1)
r = lambda *s: (torch.randn(*s, generator=gen) * 0.2).to(dev)
gw = native.GruWeights(r(3 * H, H + 1), r(3 * H, H), r(3 * H), r(3 * H))
aw = native.AggregatorWeights(r(m1, H + 1), r(m1), r(a, m1), r(g, a + 1), r(g), r(H, g), 1)
pw = native.AggregatorWeights(r(m1, H + 1), r(m1), r(a, m1), r(g, a), r(g), r(H, g), 0)
hw = native.HeadWeights(r(c, H), r(c), r(1, c), 'sigmoid')
state = torch.randn(E, H, device=dev) * 0.5
h = torch.randn(E, H, device=dev) * 0.5
am = torch.ones(p.B, dtype=torch.uint8, device=dev)
p.refresh_edge_mask()

f_gru = 2.0 * E * 3 * H * ((H + 1) + H)
f_agg = 2.0 * E * ((H + 1) * m1 + m1 * a + (a + 1) * g + g * H)
f_pred = 2.0 * E * ((H + 1) * m1 + m1 * a) + 2.0 * V * (a * g + g * H + H * c + c)


def sweep():
    out = p.neural_aggregate_edges(aw, True, state, p.edge_mask, am, h)
    p.neural_aggregate_edges(aw, False, state, p.edge_mask, am, h)
    p.neural_gru(gw, state, h, am)
    p.neural_gru(gw, state, h, am)
    p.neural_predict(pw, hw, state, p.edge_mask)
    return out


def timed(name, key, fn, flop):
    fn(); torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
    ev[0].record()
    for i in range(args.reps):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps))[args.reps // 2]
    kern = native.kernel_name(key) if key else '(all of the above)'
    print('%-22s %9.2f ms  %6.1f TFLOP/s  %.3f of peak  %s' % (name, ms, flop / ms * 1e-9, flop / (ms * 1e-3) / PEAK, kern))


print('E = %d edges, V = %d variables; widths hidden %d, mem %d, agg %d, mem_agg %d, classifier %d%s' %
      (E, V, H, m1, g, a, c, ' (PDP_NEURAL_GENERIC)' if os.environ.get('PDP_NEURAL_GENERIC') else ''))
timed('gru', 'gru', lambda: p.neural_gru(gw, state, h, am), f_gru)
timed('aggregate(by var)', 'agg_post', lambda: p.neural_aggregate_edges(aw, True, state, p.edge_mask, am, h), f_agg)
timed('aggregate(by clause)', 'agg_post', lambda: p.neural_aggregate_edges(aw, False, state, p.edge_mask, am, h), f_agg)
timed('predict', 'predict_head', lambda: p.neural_predict(pw, hw, state, p.edge_mask), f_pred)
timed('np-nd-np sweep', None, sweep, 2 * f_agg + 2 * f_gru + f_pred)
