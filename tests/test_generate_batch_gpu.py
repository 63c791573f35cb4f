"""Several sampled sequences per prompt in the device token loop (model_hip_generate_batch), GPU side, on the two Llama fixtures with graph replay on
and off; a 5-token prompt, 12 new tokens, 1, 2, 3 and 5 sequences.

1. one sequence through the batch call IS model_hip_generate_sampled with that seed: tokens and every traced logits row, bit for bit;
2. every token of every sequence is the restatement's draw (tests/sample_rule.py) from the logits the device had for that sequence at that step;
3. a sequence does not depend on where it stands in the batch, nor on its neighbours;
4. a sequence that meets the end-of-sequence token stops alone: the others go on bit for bit, with and without the host looking in;
5. the caches are right: every sequence's logits against the host-driven single-sequence loop fed that sequence's tokens;
6. m_data after the call is m_data before it, and a model_hip_generate that follows gives what it gives without the batch call.

Runs are made once per (fixture, graph, seeds, end-of-sequence token, sync) and shared between the tests."""
import os
import tempfile

import numpy as np
import pytest

import sample_rule as S
from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
pytestmark = pytest.mark.gpu
FIX = {"tiny": (llama.TINY, np.load(os.path.join(HERE, "golden", "llama_tiny.npz"))),
       "wide": (llama.TINY_WIDE, np.load(os.path.join(HERE, "golden", "llama_tiny_wide.npz")))}
PROMPT = [3, 17, 42, 5, 9]
MAX_NEW = 12
RULE = (1.0, 40, 0.95)          # temperature, top_k, top_p
DRAW_BASE = 7
A, B_, C, D_, E = 0x1234, 0xDEADBEEFCAFE, 2 ** 63 + 5, 99, 2 ** 64 - 1
SEEDS = {1: [A], 2: [A, B_], 3: [A, B_, C], 5: [A, B_, C, D_, E]}


@pytest.fixture(scope="module")
def model_dirs():
    with tempfile.TemporaryDirectory() as d:
        dirs = {}
        for name, (cfg, _) in FIX.items():
            dirs[name] = os.path.join(d, name) + "/"
            os.makedirs(dirs[name])
            llama.build_llama(DirSink(dirs[name]), cfg)
        yield dirs


def _model(model_dir, cfg, graph, upcast=True, fusion=2):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    for k, v in (("hip_autotune", 0), ("hip_fusion_level", fusion), ("hip_use_graph", graph), ("hip_resident_outputs", 0)):
        m._set_option(k, v)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, model_dir, sdpa=True, upcast=upcast)
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


_runs = {}


def run(model_dirs, which, graph, seeds, eos=-1, sync_every=0, upcast=True, fusion=2):
    """one batch call after a prefill: dict(toks, stop, trace, prompt_row)"""
    key = (which, graph, tuple(seeds), eos, sync_every, upcast, fusion)
    if key not in _runs:
        cfg = FIX[which][0]
        m = _model(model_dirs[which], cfg, graph, upcast, fusion)
        lg = llama.forward_resident(m, cfg, PROMPT, True, 0, keep_logits=True)
        toks, stop, trace, _ = llama.generate_batch(m, cfg, len(seeds), MAX_NEW, eos_id=eos, sync_every=sync_every, trace=True, temperature=RULE[0], top_k=RULE[1],
                                                    top_p=RULE[2], seeds=seeds, draw_base=DRAW_BASE)
        m.close()
        _runs[key] = dict(toks=[list(map(int, t)) for t in toks], stop=[int(s) for s in stop], trace=trace, prompt_row=lg[0, -1].copy())
    return _runs[key]


CASES = [(w, g) for w in ("tiny", "wide") for g in (0, 1)]


@pytest.mark.parametrize("which,graph", CASES)
def test_one_sequence_is_the_sampled_call(model_dirs, which, graph):
    cfg = FIX[which][0]
    R = run(model_dirs, which, graph, SEEDS[1])
    m = _model(model_dirs[which], cfg, graph)
    llama.forward_resident(m, cfg, PROMPT, True, 0, keep_logits=True)
    toks, stop, trace, _ = llama.generate(m, cfg, MAX_NEW, trace=True, temperature=RULE[0], top_k=RULE[1], top_p=RULE[2], seed=A, draw_base=DRAW_BASE)
    m.close()
    assert len(toks) == MAX_NEW and stop == 0
    assert R["toks"][0] == [int(t) for t in toks] and R["stop"] == [0]
    assert R["trace"][0].shape == trace.shape == (MAX_NEW, cfg.vocab)
    for n in range(MAX_NEW):
        assert bits(R["trace"][0][n]) == bits(trace[n]), n


@pytest.mark.parametrize("n_seq", [1, 2, 3, 5])
@pytest.mark.parametrize("which,graph", CASES)
def test_every_token_is_the_restatements_draw(model_dirs, which, graph, n_seq):
    seeds = SEEDS[n_seq]
    R = run(model_dirs, which, graph, seeds)
    ambiguous = 0
    for s in range(n_seq):
        assert len(R["toks"][s]) == MAX_NEW and R["stop"][s] == 0 and R["trace"][s].shape[0] == MAX_NEW
        for n, tok in enumerate(R["toks"][s]):
            row = R["prompt_row"] if n == 0 else R["trace"][s][n - 1]
            ambiguous += S.check(S.Prepared(row, *RULE), seeds[s], DRAW_BASE + n, tok)
    print(f"{which} graph {graph} n_seq {n_seq}: {ambiguous} ambiguous draws of {n_seq * MAX_NEW}")
    if n_seq > 1:          # (different seeds: the sequences are not all one sequence)
        assert len({tuple(t) for t in R["toks"]}) > 1


@pytest.mark.parametrize("which,graph", CASES)
def test_a_sequence_does_not_depend_on_its_place_or_its_neighbours(model_dirs, which, graph):
    R1, R2 = run(model_dirs, which, graph, [A, B_, C]), run(model_dirs, which, graph, [C, A, B_])
    for s1, s2 in ((0, 1), (1, 2), (2, 0)):
        assert R1["toks"][s1] == R2["toks"][s2] and bits(R1["trace"][s1]) == bits(R2["trace"][s2]), (s1, s2)
    # among other neighbours and in a batch of another size
    R5 = run(model_dirs, which, graph, SEEDS[5])
    for s in range(3):
        assert R1["toks"][s] == R5["toks"][s] and bits(R1["trace"][s]) == bits(R5["trace"][s]), s
    R3 = run(model_dirs, which, graph, [A, A, A])
    for s in (1, 2):
        assert R3["toks"][s] == R3["toks"][0] and bits(R3["trace"][s]) == bits(R3["trace"][0]), s
    assert R3["toks"][0] == R1["toks"][0] and bits(R3["trace"][0]) == bits(R1["trace"][0])


@pytest.mark.parametrize("which,graph", CASES)
def test_a_sequence_that_meets_the_end_stops_alone(model_dirs, which, graph):
    seeds = SEEDS[5]
    R = run(model_dirs, which, graph, seeds)
    # an end-of-sequence token that some sequence emits at a step j > 0 and that at least one other sequence never emits
    eos = next((t for s in range(5) for t in R["toks"][s][1:] if any(t not in R["toks"][o] for o in range(5) if o != s)), None)
    assert eos is not None, "no such token among these sequences: choose other seeds for the fixture"
    hit = [s for s in range(5) if eos in R["toks"][s]]
    assert 0 < len(hit) < 5 and any(R["toks"][s].index(eos) > 0 for s in hit)
    for sync_every in (0, 1):
        Q = run(model_dirs, which, graph, seeds, eos=eos, sync_every=sync_every)
        for s in range(5):
            if s in hit:
                n = R["toks"][s].index(eos)
                assert Q["toks"][s] == R["toks"][s][:n] and Q["stop"][s] == 1, (s, sync_every)
                assert Q["trace"][s].shape == (n, FIX[which][0].vocab) and bits(Q["trace"][s]) == bits(R["trace"][s][:n]), (s, sync_every)
            else:          # never meets it: unchanged bit for bit, whatever its neighbours did
                assert Q["toks"][s] == R["toks"][s] and Q["stop"][s] == 0 and len(Q["toks"][s]) == MAX_NEW, (s, sync_every)
                assert bits(Q["trace"][s]) == bits(R["trace"][s]), (s, sync_every)
    # every sequence ends at its first draw: the host, looking in after every pass, ends the call early -- and the outcome is the same
    first = R["toks"][0][0]
    Z0, Z1 = run(model_dirs, which, graph, [A, A], eos=first, sync_every=0), run(model_dirs, which, graph, [A, A], eos=first, sync_every=1)
    for Z in (Z0, Z1):
        assert Z["toks"] == [[], []] and Z["stop"] == [1, 1]


@pytest.mark.parametrize("upcast,fusion", [(True, 2), (False, 2), (True, 0)])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_every_sequences_logits_against_the_host_driven_loop(model_dirs, which, upcast, fusion):
    """Each sequence's tokens fed one by one through the host-driven single-sequence loop (one run() per token, its own cache): the logits of every pass
    against that sequence's trace, within the bound tests/test_llm_flow.py holds this backend's logits to against the reference fixture's -- 1e-3 of the
    fixture's largest fp32 logit (its outright bound; the second clause of its sdpa bound needs an fp32 reference, which sampled tokens do not have).
    Bit equality is not promised: the contractions of a batched pass have n_seq rows, those of the host loop one.  Measured on MI355X:
    worst 0.00e+00, 36 of 36 rows bit-equal in each of the six cases; the figures are printed."""
    cfg, z = FIX[which]
    seeds = SEEDS[3]
    R = run(model_dirs, which, 1, seeds, upcast=upcast, fusion=fusion)
    mx = max(float(np.abs(z[k]).max()) for k in z.files if k.startswith("logits32_"))
    worst, equal, total = 0.0, 0, 0
    for s in range(3):
        m = _model(model_dirs[which], cfg, 1, upcast, fusion)
        lg = llama.forward_resident(m, cfg, PROMPT, True, 0, keep_logits=True)
        assert bits(lg[0, -1]) == bits(R["prompt_row"])
        m.drop_tensor("logits")
        P = len(PROMPT)
        for n, tok in enumerate(R["toks"][s]):
            lg = llama.forward_resident(m, cfg, [tok], False, P)
            P += 1
            err = float(np.abs(lg[0, -1] - R["trace"][s][n]).max()) / mx
            worst, equal, total = max(worst, err), equal + (bits(lg[0, -1]) == bits(R["trace"][s][n])), total + 1
            assert err <= 1e-3, (s, n, err)
        m.close()
    print(f"{which} upcast={upcast} fusion={fusion}: worst {worst:.2e} of the largest logit, {equal} of {total} rows bit-equal")


@pytest.mark.parametrize("which,graph", CASES)
def test_m_data_is_untouched_and_the_single_loop_follows_as_if_nothing_happened(model_dirs, which, graph):
    cfg = FIX[which][0]
    NC = 2 * cfg.layers

    def flow(with_batch):
        m = _model(model_dirs[which], cfg, graph)
        llama.forward_resident(m, cfg, PROMPT, True, 0, keep_logits=True)
        if with_batch:
            names = sorted(m.get_all_tensor_names())
            lg0 = m.get_tensor("logits")[0].copy()
            kv0 = [m.get_tensor_f16(f"opkv{i}") for i in range(NC)]
            toks, stop, trace, _ = llama.generate_batch(m, cfg, 3, MAX_NEW, temperature=RULE[0], top_k=RULE[1], top_p=RULE[2], seeds=SEEDS[3], draw_base=DRAW_BASE)
            assert [list(map(int, t)) for t in toks] == run(model_dirs, which, graph, SEEDS[3])["toks"]
            assert sorted(m.get_all_tensor_names()) == names
            assert m.get_tensor("logits")[0].shape == (1, len(PROMPT), cfg.vocab) and bits(m.get_tensor("logits")[0]) == bits(lg0)
            for i in range(NC):
                c = m.get_tensor_f16(f"opkv{i}")
                assert c.shape == (1, cfg.kv_heads, len(PROMPT), cfg.head_dim) and bits(c) == bits(kv0[i]), i
        toks, stop, trace, _ = llama.generate(m, cfg, 5, trace=True)
        out = (list(map(int, toks)), stop, bits(trace), bits(m.get_tensor("logits")[0]), [bits(m.get_tensor_f16(f"opkv{i}")) for i in range(NC)])
        m.close()
        return out

    assert flow(True) == flow(False)
