"""search_rules.SearchRules: one parse, one refusal table, one spec of the manifests' metadata, at every layer.

The expected strings and dicts below are literals recorded from the code before the module existed (each layer then had
its own if-ladder); no GPU is needed, every refusal fires before a device is touched."""
import types

import pytest
import torch

from tests.stage_stub import stub_worker

SIMS = 16
ALL_ON = dict(playout_cap_fast_simulations=8, playout_cap_full_prob=0.5, forced_playouts_k=2, mcts_solver=True,
              fpu_reduction=0.2, cpuct_log=1.25, kld_stop_threshold=1e-3, kld_stop_interval=4, kld_stop_min_simulations=8,
              move_visit_offset=1, move_value_cutoff=0.5, temperature_halflife=5, value_target_lambda=0.9,
              resign_threshold=-0.9, policy_surprise_weight=0.5, eval_symmetry="random")
GUMBEL_ON = dict(gumbel_considered=4, mcts_solver=True, value_target_lambda=0.9, resign_threshold=-0.9,
                 policy_surprise_weight=0.5)
RESIGN_KW = {"resign_threshold": -0.9, "resign_min_moves": 10, "resign_consecutive": 3, "resign_playthrough_fraction": 0.1,
             "resign_streak": "side"}
# what the stage handed its worker on top of the plain arguments
ALL_ON_KWARGS = {"eval_symmetry": "random", "playout_cap_fast_simulations": 8, "playout_cap_full_prob": 0.5,
                 "forced_playouts_k": 2.0, "value_target_lambda": 0.9, "mcts_solver": True, "fpu_reduction": 0.2,
                 "fpu_root_reduction": 0.2, "cpuct_log": 1.25, "cpuct_base": 19652.0, **RESIGN_KW,
                 "kld_stop_threshold": 0.001, "kld_stop_interval": 4, "kld_stop_min_simulations": 8, "move_visit_offset": 1.0,
                 "move_value_cutoff": 0.5, "temperature_halflife": 5.0, "policy_surprise_weight": 0.5}
GUMBEL_ON_KWARGS = {"gumbel_considered": 4, "gumbel_c_visit": 50.0, "gumbel_c_scale": 1.0, "value_target_lambda": 0.9,
                    "mcts_solver": True, **RESIGN_KW, "policy_surprise_weight": 0.5}
# what the worker wrote into its manifest's metadata
RESIGN_META = {"threshold": -0.9, "min_moves": 10, "consecutive": 3, "playthrough_fraction": 0.1, "streak": "side"}
ALL_ON_META = {"eval_symmetry": "random", "playout_cap": {"fast_simulations": 8, "full_prob": 0.5},
               "forced_playouts": {"k": 2.0}, "value_target": {"td_lambda": 0.9}, "mcts_solver": True,
               "puct_shape": {"fpu_reduction": 0.2, "fpu_root_reduction": 0.2, "cpuct_log": 1.25, "cpuct_base": 19652.0},
               "resign": RESIGN_META, "kld_stop": {"threshold": 0.001, "interval": 4, "min_simulations": 8},
               "move_pick": {"visit_offset": 1.0, "value_cutoff": 0.5, "temperature_halflife": 5.0},
               "policy_surprise": {"weight": 0.5}}
GUMBEL_ON_META = {"gumbel": {"considered": 4, "c_visit": 50.0, "c_scale": 1.0}, "value_target": {"td_lambda": 0.9},
                  "mcts_solver": True, "resign": RESIGN_META, "policy_surprise": {"weight": 0.5}}

# ---- the refusal texts ------------------------------------------------------------------------------------------------------
ROOT = "not the root-PUCT search ('cuda_root')"
BACKEND = {
    "surprise": f"policy surprise weighting needs the tree backend, {ROOT}: it compares the tree search's policy target with "
                "the network prior",
    "repick": f"move_visit_offset / move_value_cutoff / temperature_halflife need the tree backend, {ROOT}: they act on the "
              "tree search's root children and its per-ply move temperature",
    "halflife": f"move_visit_offset / move_value_cutoff / temperature_halflife need the tree backend, {ROOT}: they act on "
                "the tree search's root children and its per-ply move temperature",
    "kld": f"KLD-gain early stopping needs the tree backend, {ROOT}: the rule lowers the per-game budget of the tree search",
    "resign": f"resignation needs the tree backend, {ROOT}: it reads the tree search's root values in the per-ply device tail",
    "fpu": "first-play urgency / the visit-scaled cpuct are not supported with the root-PUCT search (it needs the tree backend)",
    "cpuct": "first-play urgency / the visit-scaled cpuct are not supported with the root-PUCT search (it needs the tree "
             "backend)",
    "solver": f"the MCTS-Solver needs the tree backend, {ROOT}: it marks proven results in the search tree",
    "td": f"TD(lambda) value targets need the tree backend, {ROOT}: they blend the tree search's root values",
    "gumbel": f"the Gumbel root search needs the tree backend, {ROOT}",
    "forced": f"forced playouts need the tree backend, {ROOT}",
    "cap": f"playout cap randomization needs the tree backend, {ROOT}",
    "sym": "eval_symmetry='random' needs the tree backend: the root-PUCT search ('cuda_root') evaluates children without the "
           "symmetry hook",
}
RULES = {"cap": dict(playout_cap_fast_simulations=8, playout_cap_full_prob=0.5), "forced": dict(forced_playouts_k=2.0),
         "gumbel": dict(gumbel_considered=4), "solver": dict(mcts_solver=True), "fpu": dict(fpu_reduction=0.2),
         "cpuct": dict(cpuct_log=1.25), "kld": dict(kld_stop_threshold=1e-3, kld_stop_interval=4),
         "repick": dict(move_visit_offset=1.0), "halflife": dict(temperature_halflife=5.0), "td": dict(value_target_lambda=0.9),
         "resign": dict(resign_threshold=-0.9), "surprise": dict(policy_surprise_weight=0.5), "sym": dict(eval_symmetry="random")}
SUBJECT = {"cap": "playout cap randomization is", "forced": "forced playouts are", "gumbel": "the Gumbel root search is",
           "solver": "the MCTS-Solver is", "fpu": "first-play urgency / the visit-scaled cpuct are",
           "cpuct": "first-play urgency / the visit-scaled cpuct are", "kld": "KLD-gain early stopping is",
           "repick": "visit-offset / value-cutoff move selection is", "surprise": "policy surprise weighting is"}
WAVES, SEVERAL = "batch_k > 1 (legacy waves)", "several networks in one search"
EXTERNAL, PERSISTENT = "an external evaluator (split-phase path)", "the persistent search kernel (LZ_TREE_PERSISTENT)"
# (rule, context, extra options) -> the cause the "not supported with" message names
CAUSES = [(rule, ctx, {}, why) for rule in ("cap", "forced", "gumbel", "solver", "kld")
          for ctx, why in ((dict(batch_k=2), WAVES), (dict(several_networks=True), SEVERAL), (dict(fused=False), EXTERNAL),
                           (dict(persistent=True), PERSISTENT))] + \
         [(rule, ctx, {}, why) for rule in ("fpu", "cpuct")
          for ctx, why in ((dict(batch_k=2), WAVES), (dict(fused=False), EXTERNAL), (dict(persistent=True), PERSISTENT))] + [
    ("fpu", {}, dict(gumbel_considered=4), "the Gumbel root search (its root level has a rule of its own)"),
    ("cpuct", {}, dict(gumbel_considered=4), "the Gumbel root search (its root level has a rule of its own)"),
    ("kld", {}, dict(gumbel_considered=4), "the Gumbel root search (its Sequential Halving schedule is a function of a fixed "
                                           "budget)"),
    ("repick", {}, dict(gumbel_considered=4), "the Gumbel root search (its pick is the Sequential Halving winner and ignores "
                                              "temperatures by definition)"),
    ("repick", dict(sample_moves=False), {}, "sample_moves=False (the most visited move is played already; there is no "
                                             "sampled move to re-pick)"),
    ("gumbel", {}, dict(forced_playouts_k=2.0), "forced playouts (two rules for the same root level)"),
    ("gumbel", dict(policy_target_temperature=0.5), {}, "policy_target_temperature (the training target is not made of visit "
                                                        "counts)"),
    ("gumbel", dict(policy_target_prior_pseudocount=0.5), {}, "policy_target_prior_pseudocount > 0 (the training target is "
                                                              "not made of visit counts)"),
    ("surprise", dict(device_tail=False), {}, "the host loop (device_tail=False): the surprises and the resampling live in "
                                              "the per-ply device tail"),
    ("surprise", dict(prior_evaluator=True), {}, "a PriorEvaluator: it returns priors of its own making, there is no plain "
                                                 "network to evaluate the root with"),
]
WHOLE = [("resign", dict(device_tail=False), "resignation needs device_tail: the rule runs in the per-ply device tail, the "
                                             "host loop has none"),
         ("td", dict(device_tail=False), "value_target_lambda < 1 needs device_tail: the host loop keeps the reference's "
                                         "finalisation (every row gets the final result)"),
         ("sym", dict(batch_k=2), "eval_symmetry is not supported by the legacy waves (batch_k > 1): their wave kernels "
                                  "evaluate leaves without the symmetry hook")]


def test_every_refusal_has_the_recorded_text():
    from liuzhou_amd.search_rules import SearchRules
    for rule, kw in RULES.items():
        rules = SearchRules.parse(SIMS, **kw)
        assert rules.refusal(search_backend="cuda_root") == BACKEND[rule], rule
        for backend in ("tree", "portable", " Tree "):
            assert rules.refusal(search_backend=backend) is None
        # nothing in the way, and nothing asked about: no refusal
        assert rules.refusal() is None
        assert rules.refusal(batch_k=1, several_networks=False, fused=True, persistent=False, sample_moves=True,
                             device_tail=True, prior_evaluator=False, policy_target_temperature=None,
                             policy_target_prior_pseudocount=0.0) is None
    for rule, ctx, more, why in CAUSES:
        assert SearchRules.parse(SIMS, **RULES[rule], **more).refusal(**ctx) == f"{SUBJECT[rule]} not supported with {why}"
    for rule, ctx, text in WHOLE:
        assert SearchRules.parse(SIMS, **RULES[rule]).refusal(**ctx) == text
    # off: no configuration is refused; an unknown context key or option is a programming error
    off = SearchRules.parse(SIMS)
    assert off.refusal(search_backend="cuda_root", batch_k=2, several_networks=True, fused=False, persistent=True,
                       sample_moves=False, device_tail=False, prior_evaluator=True, policy_target_temperature=0.5,
                       policy_target_prior_pseudocount=0.5) is None
    with pytest.raises(TypeError):
        off.refuse(backend="tree")
    with pytest.raises(TypeError):
        SearchRules.parse(SIMS, gumbel=4)


# ---- the same refusal at every layer ------------------------------------------------------------------------------------------
WORKER = dict(worker_idx=0, shard_device="cuda:0", shard_games=4, seed=1, model_state_path="none.pt", output_path="none",
              mcts_simulations=SIMS, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
              exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
              opening_random_moves=0, max_game_plies=8, concurrent_games_per_device=4)
RUN = dict(num_games=2, mcts_simulations=SIMS, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
           exploration_weight=1.0, device="cuda:0")
ENGINE_NAMES = {"playout_cap_fast_simulations": "fast_simulations", "playout_cap_full_prob": "full_prob", "mcts_solver": "solver"}


def _layers(tmp_path, fused=True, **kw):
    """The four layers as callables of one configuration (flat names; the engine gets its own names)."""
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.self_play_stage import run_self_play_stage
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator, self_play_tree_gpu
    net = PriorEvaluator(lambda planes, packed: None)
    if fused:                                                    # a FusedNet by type only: a refusal comes before any use
        net = object.__new__(FusedNet)
        net.pack = types.SimpleNamespace(channels=64)
    backend = kw.pop("search_backend", "tree")
    shared = {k: kw.pop(k) for k in ("sample_moves", "policy_target_temperature", "policy_target_prior_pseudocount") if k in kw}
    eng = {ENGINE_NAMES.get(k, k): v for k, v in kw.items() if not k.startswith("kld_stop")}
    if "kld_stop_threshold" in kw:
        eng["kld_stop"] = parse_kld_stop(*(kw[k] for k in ("kld_stop_threshold", "kld_stop_interval") if k in kw))
    return {
        "stage": lambda: run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                                             output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=SIMS,
                                             concurrent_games_per_device=4, worker_fn=stub_worker, in_process=True,
                                             search_backend=backend, **shared, **kw),
        "worker": lambda: run_self_play_worker(search_backend=backend, **shared, **kw, **WORKER),
        "runner": lambda: self_play_tree_gpu(net, **shared, **kw, **RUN),
        "engine": lambda: PortableTreeMCTS(net, 4, SIMS, "cuda:0", **shared, **eng),
    }


EVERY_LAYER = [
    (dict(move_visit_offset=1.0, sample_moves=False), f"{SUBJECT['repick']} not supported with sample_moves=False (the most "
     "visited move is played already; there is no sampled move to re-pick)"),
    (dict(gumbel_considered=4, policy_target_temperature=0.5), f"{SUBJECT['gumbel']} not supported with "
     "policy_target_temperature (the training target is not made of visit counts)"),
    (dict(gumbel_considered=4, forced_playouts_k=2.0), f"{SUBJECT['gumbel']} not supported with forced playouts (two rules for "
     "the same root level)"),
    (dict(gumbel_considered=4, kld_stop_threshold=1e-3, kld_stop_interval=4), f"{SUBJECT['kld']} not supported with the Gumbel "
     "root search (its Sequential Halving schedule is a function of a fixed budget)"),
    (dict(gumbel_considered=4, cpuct_log=1.25), f"{SUBJECT['cpuct']} not supported with the Gumbel root search (its root level "
     "has a rule of its own)"),
]


@pytest.mark.parametrize("case", range(len(EVERY_LAYER)))
def test_a_configuration_is_refused_at_every_layer(tmp_path, monkeypatch, case):
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    kw, text = EVERY_LAYER[case]
    for name, call in _layers(tmp_path, **kw).items():
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == text, name


def test_the_backend_and_the_evaluator_are_refused_where_they_are_known(tmp_path, monkeypatch):
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    for rule in ("cap", "forced", "gumbel", "solver", "kld", "td", "resign", "surprise", "repick", "halflife", "cpuct"):
        layers = _layers(tmp_path, search_backend="cuda_root", **RULES[rule])
        for name in ("stage", "worker"):                      # refused before a process is spawned or a device touched
            with pytest.raises(ValueError) as err:
                layers[name]()
            assert str(err.value) == BACKEND[rule], (rule, name)
    for rule in ("solver", "gumbel", "kld", "cpuct"):         # an external evaluator: the runner and the engine know
        layers = _layers(tmp_path, fused=False, **RULES[rule])
        for name in ("runner", "engine"):
            with pytest.raises(ValueError) as err:
                layers[name]()
            assert str(err.value) == f"{SUBJECT[rule]} not supported with {EXTERNAL}", (rule, name)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    for rule in ("gumbel", "kld", "fpu"):                     # the persistent kernel: an environment switch, every layer
        for name, call in _layers(tmp_path, **RULES[rule]).items():
            with pytest.raises(ValueError) as err:
                call()
            assert str(err.value) == f"{SUBJECT[rule]} not supported with {PERSISTENT}", (rule, name)


def test_of_two_refusals_the_recorded_one_is_reported(tmp_path, monkeypatch):
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    layers = _layers(tmp_path, search_backend="cuda_root", mcts_solver=True, kld_stop_threshold=1e-3, kld_stop_interval=4)
    for name in ("stage", "worker"):
        with pytest.raises(ValueError) as err:
            layers[name]()
        assert str(err.value) == BACKEND["kld"], name
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator, self_play_tree_gpu
    prior = PriorEvaluator(lambda planes, packed: None)
    with pytest.raises(ValueError) as err:
        PortableTreeMCTS(prior, 4, SIMS, "cuda:0", solver=True, fast_simulations=8, batch_k=2)
    assert str(err.value) == "the MCTS-Solver is not supported with batch_k > 1 (legacy waves)"
    with pytest.raises(ValueError) as err:
        self_play_tree_gpu(prior, mcts_solver=True, gumbel_considered=4, batch_k=2, **RUN)
    assert str(err.value) == "the MCTS-Solver is not supported with batch_k > 1 (legacy waves)"


# ---- kwargs, round trip, canonical off values ----------------------------------------------------------------------------------
def test_kwargs_are_what_the_stage_hands_its_worker(tmp_path, monkeypatch):
    from liuzhou_amd.search_rules import SearchRules
    monkeypatch.delenv("LZ_EVAL_SYMMETRY", raising=False)
    assert SearchRules.parse(SIMS).kwargs() == {} and SearchRules.parse(SIMS) == SearchRules()
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**kw)
    for options, want in (({}, {}), (ALL_ON, ALL_ON_KWARGS), (GUMBEL_ON, GUMBEL_ON_KWARGS)):
        rules = SearchRules.parse(SIMS, **options)
        assert rules.kwargs() == want and list(rules.kwargs()) == list(want)
        assert all(type(rules.kwargs()[k]) is type(v) for k, v in want.items())
        assert SearchRules.parse(SIMS, **rules.kwargs()) == rules
        seen.clear()
        from liuzhou_amd.self_play_stage import run_self_play_stage
        run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                            output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=SIMS,
                            concurrent_games_per_device=4, worker_fn=spy, in_process=True, search_backend="tree", **options)
        plain = {"worker_idx", "shard_device", "shard_games", "seed", "model_state_path", "output_path", "mcts_simulations",
                 "temperature_init", "temperature_final", "temperature_threshold", "exploration_weight", "dirichlet_alpha",
                 "dirichlet_epsilon", "soft_value_k", "opening_random_moves", "max_game_plies",
                 "concurrent_games_per_device", "soft_label_alpha", "sparse_ply", "sparse_top_k", "search_backend",
                 "portable_mcts_backend", "portable_cpp_threads", "policy_target_temperature",
                 "policy_target_prior_pseudocount", "sample_moves", "target_samples_per_shard", "chunk_target_bytes",
                 "chunk_output_dir", "chunk_file_prefix", "chunk_file_ext"}
        assert len(seen) == 2 and all({k: v for k, v in kw.items() if k not in plain} == want for kw in seen)


def test_every_rule_has_one_off_value():
    """Parameters of a rule that is off do not tell two configurations apart (the engine cache keys on the object)."""
    from liuzhou_amd.search_rules import SearchRules
    off = SearchRules.parse(SIMS)
    assert hash(off) == hash(SearchRules())
    for kw in (dict(kld_stop_interval=7), dict(kld_stop_interval=7, kld_stop_min_simulations=3), dict(gumbel_c_visit=10.0),
               dict(gumbel_c_scale=2.0), dict(cpuct_base=8.0), dict(playout_cap_full_prob=0.3), dict(resign_min_moves=3),
               dict(resign_streak="ply", resign_consecutive=5, resign_playthrough_fraction=0.5), dict(eval_symmetry="NONE")):
        assert SearchRules.parse(SIMS, **kw) == off, kw
    assert SearchRules.parse(SIMS, fpu_reduction=0.2, cpuct_base=8.0) == SearchRules.parse(SIMS, fpu_reduction=0.2)
    assert SearchRules.parse(SIMS, cpuct_log=1.0, cpuct_base=8.0) != SearchRules.parse(SIMS, cpuct_log=1.0)
    # the per-ply tail's rules are not the engine's: engines that differ only in them are one engine
    on = SearchRules.parse(SIMS, **ALL_ON)
    assert on.engine() == SearchRules.parse(SIMS, **{k: v for k, v in ALL_ON.items() if k not in (
        "temperature_halflife", "value_target_lambda", "resign_threshold", "policy_surprise_weight")})
    import pickle
    assert pickle.loads(pickle.dumps(on)) == on
    # every value is validated, on or off, whatever the backend
    for bad in (dict(kld_stop_interval=0), dict(gumbel_c_visit=-1.0), dict(cpuct_base=0.0), dict(playout_cap_full_prob=1.5),
                dict(resign_streak="both"), dict(temperature_halflife=-1.0), dict(policy_surprise_weight=2.0),
                dict(value_target_lambda=1.5), dict(forced_playouts_k=-1.0), dict(eval_symmetry=9),
                dict(playout_cap_fast_simulations=SIMS), dict(move_value_cutoff=3.0)):
        with pytest.raises(ValueError):
            SearchRules.parse(SIMS, **bad)


# ---- metadata and counters ------------------------------------------------------------------------------------------------------
COUNTERS = {"full_searches": 30, "fast_searches": 31, "recorded_positions": 30, "forced_playouts": 5, "pruned_visits": 7,
            "gumbel_searches": 11, "solver_proofs": 3, "solver_roots_decided": 2, "solver_pick_overrides": 1,
            "kld_stopped_searches": 4, "kld_simulations_saved": 40, "move_pick_applied": 9, "move_pick_cut_visits": 8,
            "move_pick_cut_value": 6, "move_pick_changed": 2, "resigned_games": 2, "resigned_black": 1, "resigned_white": 1,
            "playthrough_games": 1, "playthrough_would_resign": 1, "playthrough_false_positive": 0, "resign_ply_sum": 50,
            "playthrough_plies_after_would": 12, "surprise_games": 4, "surprise_rows": 28, "surprise_rows_replaced": 6,
            "surprise_sum_micro": 1400000}
MERGED_RESIGN = {**RESIGN_META, "resigned_games": 8, "resigned_black": 4, "resigned_white": 4, "playthrough_games": 4,
                 "playthrough_would_resign": 4, "playthrough_false_positive": 0, "resign_ply_sum": 200,
                 "playthrough_plies_after_would": 48, "resign_avg_ply": 25, "resign_plies_saved_estimate": 96}
MERGED_SURPRISE = {"weight": 0.5, "games": 16, "rows": 112, "rows_replaced": 24, "mean_surprise": 5600000 / 1e6 / 112}
# two workers of two chunks each: every counter four times
ALL_ON_MERGED = {"playout_cap": {"fast_simulations": 8, "full_prob": 0.5, "full_searches": 120, "fast_searches": 124},
                 "forced_playouts": {"k": 2.0, "forced_playouts": 20, "pruned_visits": 28}, "value_target": {"td_lambda": 0.9},
                 "mcts_solver": True, "puct_shape": ALL_ON_META["puct_shape"], "resign": MERGED_RESIGN,
                 "kld_stop": {"threshold": 0.001, "interval": 4, "min_simulations": 8, "kld_stopped_searches": 16,
                              "kld_simulations_saved": 160},
                 "move_pick": {"visit_offset": 1.0, "value_cutoff": 0.5, "temperature_halflife": 5.0, "move_pick_applied": 36,
                               "move_pick_cut_visits": 32, "move_pick_cut_value": 24, "move_pick_changed": 8},
                 "policy_surprise": MERGED_SURPRISE}
GUMBEL_ON_MERGED = {"gumbel": {"considered": 4, "c_visit": 50.0, "c_scale": 1.0, "gumbel_searches": 44},
                    "value_target": {"td_lambda": 0.9}, "mcts_solver": True, "resign": MERGED_RESIGN,
                    "policy_surprise": MERGED_SURPRISE}
RULE_META_KEYS = ("eval_symmetry", "playout_cap", "forced_playouts", "gumbel", "value_target", "mcts_solver", "puct_shape",
                  "resign", "kld_stop", "move_pick", "policy_surprise")


def _reporting_worker(meta, counters):
    """The stub worker as the real one reports the rules: `meta` in its metadata, `counters` in its stats."""
    import tests.stage_stub as S
    from liuzhou_amd import self_play_worker as W

    def worker(**kw):
        orig = W.write_worker_chunks

        def write(run_once, **a):
            a["meta_common"] = {**a["meta_common"], **meta}

            def counted(n):
                batch, st = run_once(n)
                st.mcts_counters.update(counters)
                return batch, st
            return orig(counted, **a)
        S.write_worker_chunks = write
        try:
            return S.stub_worker(**kw)
        finally:
            S.write_worker_chunks = orig
    return worker


def test_meta_and_the_merged_manifest(tmp_path, monkeypatch):
    from liuzhou_amd.search_rules import SearchRules
    from liuzhou_amd.self_play_stage import run_self_play_stage
    monkeypatch.delenv("LZ_EVAL_SYMMETRY", raising=False)
    assert SearchRules.parse(SIMS).meta() == {}
    for options, meta, merged in ((ALL_ON, ALL_ON_META, ALL_ON_MERGED), (GUMBEL_ON, GUMBEL_ON_META, GUMBEL_ON_MERGED)):
        rules = SearchRules.parse(SIMS, **options)
        assert rules.meta() == meta and list(rules.meta()) == list(meta)
        _, manifest = run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                                          output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=SIMS,
                                          concurrent_games_per_device=4, worker_fn=_reporting_worker(rules.meta(), COUNTERS),
                                          in_process=True, search_backend="tree", **options)
        got = {k: manifest["metadata"][k] for k in RULE_META_KEYS if k in manifest["metadata"]}
        assert got == merged and list(got) == list(merged)
    # the re-pick's counters are copied only where the re-pick ran (the half-life alone has none)
    half = SearchRules.parse(SIMS, temperature_halflife=5.0)
    _, manifest = run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                                      output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=SIMS,
                                      concurrent_games_per_device=4, worker_fn=_reporting_worker(half.meta(), {}),
                                      in_process=True, search_backend="tree", temperature_halflife=5.0)
    assert manifest["metadata"]["move_pick"] == {"visit_offset": 0.0, "value_cutoff": 0.0, "temperature_halflife": 5.0}


def test_the_engine_counters_of_the_rules_that_are_on():
    from liuzhou_amd.search_rules import SearchRules, engine_counters

    class Engine:
        cap_counts = torch.tensor([30, 31])
        forced_counts = torch.tensor([5, 7])
        gumbel_searches = torch.tensor([11])
        solver_counts = torch.tensor([3, 2, 1])
        kld_counts = torch.tensor([4, 40])
        move_pick_counts = torch.tensor([9, 8, 6, 2])
    engine_keys = ("full_searches", "fast_searches", "forced_playouts", "pruned_visits", "gumbel_searches", "solver_proofs",
                   "solver_roots_decided", "solver_pick_overrides", "kld_stopped_searches", "kld_simulations_saved",
                   "move_pick_applied", "move_pick_cut_visits", "move_pick_cut_value", "move_pick_changed")
    assert engine_counters(SearchRules.parse(SIMS), Engine) == {}
    got = engine_counters(SearchRules.parse(SIMS, **ALL_ON), Engine)
    assert got == {k: COUNTERS[k] for k in engine_keys if k != "gumbel_searches"}
    got = engine_counters(SearchRules.parse(SIMS, **GUMBEL_ON), Engine)
    assert got == {k: COUNTERS[k] for k in ("gumbel_searches", "solver_proofs", "solver_roots_decided", "solver_pick_overrides")}
    assert engine_counters(SearchRules.parse(SIMS, temperature_halflife=5.0), Engine) == {}
    assert all(type(v) is int for v in got.values())
