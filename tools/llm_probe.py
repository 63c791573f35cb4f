"""Dev tool (GPU box): the LLM flow (synth/llama.py, src/llm.cpp's loop shape) at TinyLlama-1.1B size -- 22 layers, hidden 2048, 32 query / 4 key-value
heads of 64, MLP 5632, vocabulary 32000, random weights -- prefill of 32 tokens, then greedy decode; wall ms per call, caches resident in the Model (fp16, renamed).
--generate: instead, the host-driven resident loop against the device loop (Model.generate) in one process, 64 tokens each (profiles/llm_generate_probe.txt).
--generate --temperature T [--top-k K] [--top-p P] [--seed S]: the device loop greedy (twice: their difference is the noise) against the same loop sampling
by that rule, then osg_decode_sample alone at V = 32000 and 128256; each option takes a comma-separated list, one entry per rule
(profiles/llm_generate_sampled_probe.txt: --temperature 0.8,1 --top-k 40,0 --top-p 0.9,0.95).
--generate --sequences N[,N...] [--temperature T] [--top-k K] [--top-p P] [--seed S]: the single sampled loop (Model.generate) as the baseline, then
Model.generate_batch with each N, 64 tokens per sequence after the 32-token prefill, all in one process: ms per pass and tokens per second
(profiles/llm_generate_batch_probe.txt: --sequences 1,2,4,8,16 --temperature 0.8 --top-k 40 --top-p 0.9).
--generate --penalties [--off-only] [--seed S]: the warm sampled loop (T 0.8, top_k 40, top_p 0.9) with the four controls off and with
repetition 1.1, presence 0.2, frequency 0.1, min_p 0.05 over a 32-token history (the prompt), alternating, five calls each after one cold call: ms per
token of every call, the range of each leg and the difference of the medians.  --off-only runs the controls-off calls alone, which a library of an older
tree can run too (OSA_LIB_HOST names its host library, its libosgpu.so beside it): the A/B of profiles/llm_generate_penalties_probe.txt.
--turn: two chat turns of 32 prompt tokens and 64 generated tokens each, chunk 32: Model.turn (prefill and loop on the device, one call per turn) against
forward_resident + Model.generate on the same tokens, three conversations each way in one process: wall and device ms per turn, plans built
(profiles/llm_turn_probe.txt)."""
import os, sys, time, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onnxstream_amd import build as b
from onnxstream_amd.bindings import Model
from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

cfg = llama.LlamaConfig(vocab=32000, hidden=2048, layers=22, heads=32, kv_heads=4, inter=5632, max_pos=2048, name="tinyllama_1b")
d = os.path.join(os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth"), cfg.name) + "/"
if not os.path.exists(d + ".complete"):
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    llama.build_llama(DirSink(d), cfg)
    open(d + ".complete", "w").write("ok")
    print(f"emitted {cfg.name} in {time.time()-t0:.1f} s", flush=True)

def generate_leg(n_new=64):
    """--generate: ms per token of the host-driven resident loop (one run() per token: re-plan, 3 int64 inputs up, logits down, argmax on the host) against
    the device loop (Model.generate: one call, one kept plan, one synchronisation) in the same process, n_new tokens after the 32-token prefill; greedy
    tokens must agree.  The device loop is timed cold (the call that builds and captures its plan) and warm (a second prompt, the plan kept)."""
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab, 32)]

    def fresh():
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m._set_option("hip_autotune", 0)
        m._set_option("hip_resident_outputs", 1)
        m.add_outputs_convert("logits")
        llama.configure(m, cfg, d, sdpa=True, upcast=True)
        return m

    m = fresh()
    lg = llama.forward_resident(m, cfg, prompt, True, 0)
    host_toks, times, dev, P = [], [], [], len(prompt)
    t_all = time.perf_counter()
    for k in range(n_new):
        nxt = int(np.argmax(lg[0, -1]))
        host_toks.append(nxt)
        t0 = time.perf_counter()
        lg = llama.forward_resident(m, cfg, [nxt], False, P)
        times.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.hip_last_pass_ms())
        P += 1
    host_ms = (time.perf_counter() - t_all) * 1e3 / n_new
    print(f"host-driven loop, {n_new} tokens after a {len(prompt)}-token prefill: wall {host_ms:.2f} ms/token (median call {np.median(times):.2f}, min {min(times):.2f}), "
          f"device {np.median(dev):.2f} ms/pass, {m.hip_last_kernel_count()} launches per token + 1 synchronisation, plans built {m.hip_plans_built()}", flush=True)
    m.close()

    m = fresh()
    for leg in ("cold (builds and captures the plan)", "warm (plan kept)"):
        m.clear_tensors()
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        built = m.hip_plans_built()
        t0 = time.perf_counter()
        toks, stop, _, ms = llama.generate(m, cfg, n_new)
        wall = (time.perf_counter() - t0) * 1e3
        agree = sum(int(a == c) for a, c in zip(toks, host_toks))
        print(f"device loop {leg}: wall {wall / n_new:.2f} ms/token ({wall:.1f} ms the call), device {ms / n_new:.2f} ms/token, {len(toks)} tokens, stop {stop}, "
              f"{agree} of {n_new} tokens equal the host loop's, plans built by the call {m.hip_plans_built() - built}, "
              f"{m.hip_last_kernel_count()} kernels per pass inside one graph launch: 2 host launches per token (pick + graph), 1 synchronisation per call", flush=True)
    print(m.hip_decode_plan_info().splitlines()[0], flush=True)
    m.close()


def _option(name, default, conv):
    if name not in sys.argv:
        return None if default is None else [default]
    return [conv(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")]


def sampled_leg(rules, seed, n_new=64):
    """--generate --temperature ...: warm device-loop calls of n_new tokens after the 32-token prefill in one process -- greedy, greedy again, then one per
    sampling rule -- and the sampling kernel by itself: the mean of 100 back-to-back launches between two events, over a row of N(0, 3^2) logits."""
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab, 32)]
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m._set_option("hip_autotune", 0)
    m._set_option("hip_resident_outputs", 1)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, d, sdpa=True, upcast=True)

    def leg(name, **kw):
        m.clear_tensors()
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        built = m.hip_plans_built()
        t0 = time.perf_counter()
        toks, stop, _, ms = llama.generate(m, cfg, n_new, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        print(f"device loop {name}: wall {wall / n_new:.3f} ms/token ({wall:.1f} ms the call), device {ms / n_new:.3f} ms/token, {len(toks)} tokens "
              f"({len(set(int(t) for t in toks))} distinct), stop {stop}, plans built by the call {m.hip_plans_built() - built}", flush=True)

    leg("greedy, cold (builds and captures the plan)")
    leg("greedy, warm, first")
    leg("greedy, warm, second")
    for t, k, p in rules:
        leg(f"sampled T {t:g} top_k {k} top_p {p:g} seed {seed}, warm", temperature=t, top_k=k, top_p=p, seed=seed)
    leg("greedy, warm, third")
    print(m.hip_decode_plan_info().splitlines()[0], flush=True)
    m.close()

    from onnxstream_amd import osgpu
    g = osgpu.Gpu(0)
    reps = 100
    for V in (32000, 128256):
        row = g.to_dev((np.random.default_rng(V).standard_normal((1, V)) * 3).astype(np.float32))
        ids, pos, toks = g.to_dev(np.zeros(1, np.int64)), g.to_dev(np.zeros(1, np.int64)), g.to_dev(np.zeros(reps + 8, np.int64))
        for t, k, p in rules:
            state = g.to_dev(np.array([0, 1, 0, 0], np.int32))
            for _ in range(8):
                g.decode_sample(row, -1, state, ids, pos, toks, t, k, p, seed)
            g.sync()
            g.timer_start()
            for _ in range(reps):
                g.decode_sample(row, -1, state, ids, pos, toks, t, k, p, seed)
            us = g.timer_stop() * 1e3 / reps
            print(f"osg_decode_sample alone, V {V}, T {t:g} top_k {k} top_p {p:g}: {us:.1f} us per launch (mean of {reps} back to back), "
                  f"{int(state.numpy()[2])} tokens taken", flush=True)
        state = g.to_dev(np.array([0, 1, 0, 0], np.int32))
        for _ in range(8):
            g.decode_pick(row, -1, state, ids, pos, toks)
        g.sync()
        g.timer_start()
        for _ in range(reps):
            g.decode_pick(row, -1, state, ids, pos, toks)
        print(f"osg_decode_pick alone, V {V}: {g.timer_stop() * 1e3 / reps:.1f} us per launch (mean of {reps} back to back)", flush=True)
    g.close()


def penalties_leg(seed, off_only, n_new=64, repeats=5):
    """--generate --penalties: warm device-loop calls of n_new tokens after the 32-token prefill in one process, the controls off and on in turn; the
    range of the controls-off calls among themselves is the noise the difference is read against."""
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab, 32)]
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m._set_option("hip_autotune", 0)
    m._set_option("hip_resident_outputs", 1)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, d, sdpa=True, upcast=True)
    rule = dict(temperature=0.8, top_k=40, top_p=0.9, seed=seed)
    controls = dict(repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=0.1, min_p=0.05, history=prompt)

    def leg(name, **kw):
        m.clear_tensors()
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        built = m.hip_plans_built()
        t0 = time.perf_counter()
        toks, stop, _, ms = llama.generate(m, cfg, n_new, **rule, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        print(f"sampled loop, {name}: device {ms / n_new:.4f} ms/token, wall {wall / n_new:.4f} ms/token, {len(toks)} tokens ({len(set(int(t) for t in toks))} distinct), "
              f"stop {stop}, plans built by the call {m.hip_plans_built() - built}", flush=True)
        return ms / n_new

    print(f"host library {os.path.basename(os.path.dirname(b.LIB_HOST))}/{os.path.basename(b.LIB_HOST)}", flush=True)
    leg("controls off, cold (builds and captures the plan)")
    off, on = [], []
    for r in range(repeats):
        off.append(leg(f"controls off, warm {r}"))
        if not off_only:
            on.append(leg(f"controls on (1.1, 0.2, 0.1, min_p 0.05, history 32), warm {r}", **controls))
    print(f"controls off: min {min(off):.4f} median {np.median(off):.4f} max {max(off):.4f} ms/token over {repeats} calls", flush=True)
    if on:
        print(f"controls on:  min {min(on):.4f} median {np.median(on):.4f} max {max(on):.4f} ms/token over {repeats} calls; median on - median off "
              f"{np.median(on) - np.median(off):+.4f} ms/token ({(np.median(on) / np.median(off) - 1) * 100:+.2f} %)", flush=True)
    m.close()


def batch_leg(n_list, rule, seed, n_new=64):
    """--generate --sequences ...: per N a cold call (the decode plan of batch N is built and captured) and two warm ones; before, between and after them the
    single-sequence sampled loop, whose calls among themselves show the run-to-run spread.  No sequence can stop (eos -1): every call is n_new passes."""
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab, 32)]
    t, k, p = rule
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m._set_option("hip_autotune", 0)
    m._set_option("hip_resident_outputs", 1)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, d, sdpa=True, upcast=True)

    def prefill():
        m.clear_tensors()
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        return m.hip_plans_built()

    def single(name):
        built = prefill()
        t0 = time.perf_counter()
        toks, stop, _, ms = llama.generate(m, cfg, n_new, temperature=t, top_k=k, top_p=p, seed=seed)
        wall = (time.perf_counter() - t0) * 1e3
        print(f"single sampled loop, {name}: device {ms / n_new:.3f} ms/pass, {n_new / ms * 1e3:.0f} tokens/s, wall {wall:.1f} ms the call, {len(toks)} tokens, "
              f"plans built by the call {m.hip_plans_built() - built}", flush=True)
        return [int(x) for x in toks]

    def batch(n, name):
        built = prefill()
        t0 = time.perf_counter()
        toks, stop, _, ms = llama.generate_batch(m, cfg, n, n_new, temperature=t, top_k=k, top_p=p, seed=seed)
        wall = (time.perf_counter() - t0) * 1e3
        total = sum(len(x) for x in toks)
        print(f"batch loop --sequences {n}, {name}: device {ms / n_new:.3f} ms/pass, {total / ms * 1e3:.0f} tokens/s, wall {wall:.1f} ms the call, {total} tokens "
              f"({len(set(tuple(int(v) for v in x) for x in toks))} distinct sequences), plans built by the call {m.hip_plans_built() - built}, "
              f"{m.hip_last_kernel_count()} kernels per pass", flush=True)
        return [[int(v) for v in x] for x in toks]

    print(f"rule: T {t:g} top_k {k} top_p {p:g}, seeds {seed} + s; {n_new} passes per call after a {len(prompt)}-token prefill", flush=True)
    single("cold (builds and captures the plan)")
    base = single("warm, first")
    single("warm, second")
    for n in n_list:
        batch(n, "cold (builds and captures the plan)")
        got = batch(n, "warm, first")
        batch(n, "warm, second")
        print(f"    sequence 0 of the batch equals the single loop with its seed: {got[0] == base}", flush=True)
        print("    " + m.hip_decode_plan_info().splitlines()[0], flush=True)
    single("cold again (the plan of one sequence is rebuilt)")
    single("warm, third")
    single("warm, fourth")
    m.close()


def turn_leg(n_prompt=32, n_new=64, chunk=32, repeats=3):
    """--turn: two chat turns (n_prompt prompt tokens then n_new generated, twice) through Model.turn against forward_resident + Model.generate on the
    same tokens, in one process: wall and device ms per turn, and the plans each way builds.  Every way runs `repeats` conversations; the spread
    between two repeats of the baseline is the noise the difference is read against."""
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, cfg.vocab, n_prompt)] for _ in range(2)]
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m._set_option("hip_autotune", 0)
    m._set_option("hip_resident_outputs", 1)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, d, sdpa=True, upcast=True)
    llama.forward_resident(m, cfg, [1], True, 0)      # the weight-loading pass
    capacity = 2 * (n_prompt + n_new)

    def baseline():
        m.clear_tensors()
        P, out, walls, devs = 0, [], [], []
        for k, prompt in enumerate(prompts):
            t0 = time.perf_counter()
            llama.forward_resident(m, cfg, prompt, k == 0, P, keep_logits=True)
            dev = m.hip_last_pass_ms()
            toks, stop, _, ms = llama.generate(m, cfg, n_new)
            walls.append((time.perf_counter() - t0) * 1e3)
            devs.append(dev + ms)
            m.drop_tensor("logits")
            P += len(prompt) + len(toks)
            out.append([int(t) for t in toks])
        return out, walls, devs

    def device():
        m.clear_tensors()
        out, walls, devs = [], [], []
        for k, prompt in enumerate(prompts):
            t0 = time.perf_counter()
            toks, stop, _, ms = llama.turn(m, cfg, prompt, n_new, chunk=chunk, capacity=capacity, first=k == 0)
            walls.append((time.perf_counter() - t0) * 1e3)
            devs.append(ms)
            out.append([int(t) for t in toks])
        return out, walls, devs

    ref = None
    for name, leg in (("forward_resident + generate", baseline), ("turn", device)):
        for r in range(repeats):
            built = m.hip_plans_built()
            toks, walls, devs = leg()
            ref = ref or toks
            same = sum(int(a == c) for x, y in zip(toks, ref) for a, c in zip(x, y))
            print(f"{name}, repeat {r}: turn 1 wall {walls[0]:.1f} ms device {devs[0]:.1f} ms; turn 2 wall {walls[1]:.1f} ms device {devs[1]:.1f} ms; "
                  f"{sum(len(t) for t in toks)} tokens, {same} equal the first baseline's; plans built {m.hip_plans_built() - built}", flush=True)
    print(m.hip_prefill_plan_info().splitlines()[0] + "; " + m.hip_decode_plan_info().splitlines()[0], flush=True)
    m.close()


if "--turn" in sys.argv:
    turn_leg()
    sys.exit(0)

if "--generate" in sys.argv:
    temps = _option("--temperature", None, float)
    seqs = _option("--sequences", None, int)
    if "--penalties" in sys.argv:
        penalties_leg(_option("--seed", 0, int)[0], "--off-only" in sys.argv)
    elif seqs is not None:
        rule = ((temps or [0.8])[0], _option("--top-k", 40, int)[0], _option("--top-p", 0.9, float)[0])
        batch_leg(seqs, rule, _option("--seed", 0, int)[0])
    elif temps is None:
        generate_leg()
    else:
        ks, ps, seed = _option("--top-k", 0, int), _option("--top-p", 1.0, float), _option("--seed", 0, int)[0]
        ks, ps = (ks * len(temps))[:len(temps)] if len(ks) == 1 else ks, (ps * len(temps))[:len(temps)] if len(ps) == 1 else ps
        sampled_leg(list(zip(temps, ks, ps)), seed)
    sys.exit(0)

for sdpa in (True, False):
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m._set_option("hip_autotune", 0)
    m.add_outputs_convert("logits")
    if os.environ.get("LLM_RESIDENT_OUTPUTS") == "1":      # the caches never leave the device (Model::m_hip_resident_outputs)
        m._set_option("hip_resident_outputs", 1)
    llama.configure(m, cfg, d, sdpa=sdpa, upcast=True)
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab, 32)]
    t0 = time.perf_counter()
    lg = llama.forward_resident(m, cfg, prompt, True, 0)
    t1 = time.perf_counter()
    print(f"sdpa={sdpa}: first call (weights become resident, prefill 32 tokens): {(t1-t0)*1e3:.0f} ms, plan {m.hip_last_kernel_count()} launches, device {m.hip_last_pass_ms():.2f} ms", flush=True)
    times, dev = [], []
    P = len(prompt)
    for k in range(24):
        nxt = int(np.argmax(lg[0, -1]))
        t0 = time.perf_counter()
        lg = llama.forward_resident(m, cfg, [nxt], False, P)
        times.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.hip_last_pass_ms())
        P += 1
    assert np.isfinite(lg).all()
    print(f"sdpa={sdpa}: decode wall ms/token median {np.median(times):.1f} (min {min(times):.1f}), device ms/token median {np.median(dev):.2f}, launches {m.hip_last_kernel_count()}", flush=True)
    m.close()
