"""Worker HTTP service: one process per MI355X (or a CPU worker), API-compatible with the
reference's Flask worker (``worker/app.py``):

    GET  /health         {"status":"healthy","resources":{cpu,memory,gpu,gpu_available,device},
                          "loaded_models","loaded_tokenizers","loaded_shards"}
    POST /load_model     {model_name}
    POST /load_shard     {model_name, shard_id, shard_path}
    POST /unload_model   {model_name}
    POST /inference      {model_name, prompt, max_length=100, shard_ids?, timeout=60}
                         -> {"status":"success","result","execution_time"}; 408 on timeout
    POST /ssh_setup      {host, port=22, username, password | key_path}

Differences that fix reference defects:
* ``gpu`` is the real HBM-in-use fraction of this worker's device (the reference reported
  memory_allocated / max_memory_allocated, W3);
* ``shard_id = 0`` is accepted (W5 rejected it via ``all([...])``);
* ``/load_shard`` really loads the stage's weights (C++ safetensors -> hipMemcpyAsync);
* ``/inference`` with ``shard_ids`` runs ALL listed shards as a pipeline (loopback on this
  GPU, or the multi-GPU ring when this worker heads one) and refuses a set of shards that
  does not cover the model, instead of running shard 0 as if it were the whole model (W8);
* the deadline is enforced inside the decode loop (every step), not only before/after;
* concurrent requests are continuously batched by an engine thread (EngineService).
"""
from __future__ import annotations

import logging
import os
import socket
import threading
import time
from functools import wraps
from pathlib import Path
from typing import Dict, Optional

import psutil
import torch
from flask import Flask, jsonify, request

from ..config import Settings, get_settings
from ..engine.sequence import SamplingParams
from ..models.configs import get_config
from ..shard.writer import load_shard, read_metadata, stage_plan_from_metadata
from ..utils import faults
from ..utils.log import setup_logging
from .service import EngineService, PipelineFailed

log = logging.getLogger("dli.worker")


def gpu_busy_percent(index: int) -> Optional[float]:
    """Device busy % from the amdgpu driver (sysfs ``gpu_busy_percent`` of the PCI device
    backing HIP device `index`); None where unavailable (reference W3 only had a memory
    ratio proxy, worker/app.py:60-67)."""
    try:
        p = torch.cuda.get_device_properties(index)
        bus = getattr(p, "pci_bus_id", None)
        if bus is None:
            return None
        dom, dev = getattr(p, "pci_domain_id", 0), getattr(p, "pci_device_id", 0)
        path = Path(f"/sys/bus/pci/devices/{dom:04x}:{bus:02x}:{dev:02x}.0/gpu_busy_percent")
        return float(path.read_text().strip()) if path.exists() else None
    except Exception:  # noqa: BLE001
        return None


class WorkerState:
    def __init__(self, settings: Settings, device: Optional[str] = None,
                 engine_kwargs: Optional[dict] = None):
        self.settings = settings
        if device is None:
            device = "cuda" if (settings.use_gpu and torch.cuda.is_available()) else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.device_str = "cuda" if self.device.type == "cuda" else "cpu"
        gpu = self.device.type == "cuda"
        self.engine_kwargs = dict(max_batch=256 if gpu else 16,
                                  max_model_len=2048 if gpu else 512,
                                  num_blocks=None if gpu else 512)
        self.engine_kwargs.update(engine_kwargs or {})
        # the KV cache's element type of every engine this worker builds (bf16 | fp8); an
        # unknown value stops the worker here, not at the first /load_model
        from ..engine.kv_cache import resolve_kv_dtype
        self.engine_kwargs["kv_dtype"] = resolve_kv_dtype(
            self.engine_kwargs.get("kv_dtype") or getattr(settings, "kv_cache_dtype", None))
        # likewise the weight dtype (bf16 | fp8; None: a checkpoint's own)
        from ..models.weights import resolve_weight_dtype
        self.engine_kwargs["weight_dtype"] = resolve_weight_dtype(
            self.engine_kwargs.get("weight_dtype") or getattr(settings, "weight_dtype", "")
            or None)
        if gpu and self.engine_kwargs.get("num_blocks") is None:
            # a worker may serve several models (/load_model per name): each engine's KV
            # pool is capped at max_batch x max_model_len tokens (DLI_KV_MAX_TOKENS
            # overrides) so the first model cannot take the HBM the next one's weights need
            kw = self.engine_kwargs
            kw.setdefault("max_kv_tokens",
                          int(os.environ.get("DLI_KV_MAX_TOKENS", "0") or 0)
                          or kw["max_batch"] * kw["max_model_len"])
        self.services: Dict[str, object] = {}           # model_name -> service
        self.tokenizers: Dict[str, object] = {}
        self.shards: Dict[str, Dict[int, dict]] = {}     # model -> shard_id -> record
        self.shard_pipes: Dict[tuple, object] = {}     # (model, shard ids) -> EngineService
        self.weights_source: Dict[str, str] = {}
        self.pipeline: Optional[dict] = None            # ring this worker joined via /load_shard
        self._pipe_engine = None
        self.lock = threading.RLock()
        # set while no ring teardown is running: a teardown drains a GPU stream and destroys
        # the process group outside the lock, and a re-forming join must not rendezvous (or
        # be torn down) under it
        self._teardown_idle = threading.Event()
        self._teardown_idle.set()
        self.data_plane: Optional[dict] = None          # resolved plane of a multi-rank engine
        os.makedirs(settings.model_cache_dir, exist_ok=True)

    # ------------------------------------------------------------------ models
    def load_model(self, name: str):
        """Reference: ``from_pretrained(name, cache_dir=MODEL_CACHE_DIR)`` then ``.to(DEVICE)``
        (worker/app.py:117-124). Here: weights from ``MODEL_CACHE_DIR/<name>/`` when present
        (a ``model.safetensors`` + ``config.json``, or the ``shard_<i>/`` directories the
        ``shard-model`` CLI writes), streamed into HBM by the C++ loader; otherwise the
        architecture's deterministic random init (no checkpoints are fetchable here)."""
        from ..engine.llm_engine import LLMEngine
        from ..shard.writer import load_cached_model
        with self.lock:
            if name in self.services or name == getattr(self, "pipeline_model", None):
                return False            # a pipeline head serves its model across all stages
            cached = load_cached_model(self.settings.model_cache_dir, name, self.device)
            if cached is not None:
                cfg, params, tok_dir = cached
                eng = LLMEngine(cfg, device=str(self.device), params=params,
                                tokenizer_path=tok_dir, **self.engine_kwargs)
                self.weights_source[name] = "cache"
            else:
                cfg = get_config(name)
                eng = LLMEngine(cfg, device=str(self.device), **self.engine_kwargs)
                self.weights_source[name] = "random-init"
            if eng.device.type == "cuda":
                eng.warmup(serving=True)   # decode graphs (+ GEMM autotune, mixed-step plans)
            self.services[name] = EngineService(eng, name=name.replace("/", "_"))
            self.tokenizers[name] = eng.tokenizer
            return True

    def unload_model(self, name: str):
        with self.lock:
            if (self.pipeline is not None and self._pipe_engine is not None
                    and name == getattr(self, "pipeline_model", None)):
                self._leave_pipeline()
            svc = self.services.pop(name, None)
            if svc is not None:
                svc.close()
            self.tokenizers.pop(name, None)
            self.shards.pop(name, None)
            for k in [k for k in self.shard_pipes if k[0] == name]:
                self.shard_pipes.pop(k).close()
            if self.device.type == "cuda":
                torch.cuda.empty_cache()

    def load_shard(self, name: str, shard_id: int, path: str):
        with self.lock:
            self.shards.setdefault(name, {})
            if shard_id in self.shards[name]:
                return False
            meta = read_metadata(path, name, shard_id)
            rec = {"path": path, "metadata": meta, "params": None, "cfg": None}
            if (Path(path) / "model.safetensors").exists():
                cfg, meta, params = load_shard(path, device=self.device)
                rec.update(metadata=meta, params=params, cfg=cfg)
            if name not in self.tokenizers:
                from ..tokenizer import load_tokenizer
                tok_dir = os.path.join(os.path.dirname(path.rstrip("/")), "tokenizer")
                try:
                    cfg = rec["cfg"] or get_config(name)
                except KeyError:
                    cfg = None
                self.tokenizers[name] = load_tokenizer(cfg, tok_dir)
            self.shards[name][shard_id] = rec
            return True

    def join_pipeline(self, name: str, shard_id: int, path: str, spec: dict) -> bool:
        """``/load_shard`` with a "pipeline" spec (the shard's layers go
        onto this GPU and the worker joins the pipeline communicator). Every node of the
        ring gets one such call: rank = shard id, ``world_size`` = the shard count of the
        export (``metadata.json``), rendezvous at ``init_method`` (``tcp://host:port``). The
        join runs in the background: the master posts to all N nodes before any of them can
        finish the rendezvous. Rank 0 then serves the model as a pipeline head and reports
        every stage as its shard (the master routes the model's requests to it); the other
        ranks run their stage loop until the head unloads the model. /health shows the
        state ("joining" -> "serving" | "failed")."""
        meta = read_metadata(path, name, shard_id)
        world = int(spec.get("world_size") or meta.get("num_shards") or 0)
        init_method = spec.get("init_method")
        if world < 2 or not init_method:
            raise ValueError("pipeline spec needs init_method and world_size >= 2")
        if not 0 <= shard_id < world:
            raise ValueError(f"shard {shard_id} outside a {world}-stage pipeline")
        while True:
            if not self._teardown_idle.wait(timeout=120.0):
                raise RuntimeError("the previous ring is still tearing down; retry later")
            with self.lock:
                if not self._teardown_idle.is_set():
                    continue                        # a teardown started meanwhile
                if (self.pipeline is not None
                        and self.pipeline["state"] in ("joining", "serving")):
                    if (self.pipeline["model_name"], self.pipeline["rank"]) == (name, shard_id):
                        return False
                    raise ValueError(f"this worker already serves stage "
                                     f"{self.pipeline['rank']} of "
                                     f"{self.pipeline['model_name']}")
                if self.pipeline is not None:       # failed / stopped: re-form from scratch
                    self._clear_pipeline()
                self.pipeline = {"model_name": name, "rank": shard_id, "world_size": world,
                                 "init_method": init_method, "state": "joining",
                                 "error": None}
                break
        shard_dir = os.path.dirname(path.rstrip("/"))
        threading.Thread(target=self._join, args=(name, shard_id, world, init_method,
                                                  shard_dir), daemon=True,
                         name=f"dli-join-{name}-{shard_id}").start()
        return True

    def _join(self, name, rank, world, init_method, shard_dir):
        from ..parallel.pipeline import DistributedPipelineEngine
        from ..parallel.transport import init_distributed
        from .service import PipelineService
        rec = self.pipeline
        eng = None
        try:
            cuda = self.device.type == "cuda"
            if cuda:
                torch.cuda.set_device(self.device)
            init_distributed(device=self.device if cuda else None, init_method=init_method,
                             world_size=world, rank=rank)
            kw = self.engine_kwargs
            eng = DistributedPipelineEngine(name, self.device, max_batch=kw["max_batch"],
                                            max_model_len=kw["max_model_len"],
                                            num_blocks=kw["num_blocks"], shard_dir=shard_dir,
                                            dtype=_shard_dtype(shard_dir, rank),
                                            max_kv_tokens=kw.get("max_kv_tokens") or 0,
                                            kv_dtype=kw.get("kv_dtype"),
                                            weight_dtype=kw.get("weight_dtype"))
            eng.warmup()
            self._pipe_engine = eng
            ch = eng.channel
            rec["data_plane"] = ch.data_plane
            rec["control_plane"] = ch.ctrl_kind
            if ch.fallback:
                rec["data_plane_fallback"] = ch.fallback
            self.data_plane = {"kind": "pipeline", "plane": ch.data_plane,
                               "control": ch.ctrl_kind, "fallback": ch.fallback,
                               "ranks": ch.world}
            if rank == 0:
                with self.lock:
                    self.tokenizers[name] = eng.head.tok
                    self.pipeline_shards = [
                        {"model_name": name, "shard_id": p.shard_id,
                         "path": os.path.join(shard_dir, f"shard_{p.shard_id}"),
                         "metadata": read_metadata(os.path.join(shard_dir,
                                                                f"shard_{p.shard_id}"),
                                                   name, p.shard_id)}
                        for p in eng.plans]
                    self.pipeline_service = PipelineService(
                        eng, name=name.replace("/", "_"), on_failure=self._pipeline_failed)
                    self.pipeline_model = name
                    rec["state"] = "serving"
                return
            rec["state"] = "serving"
            eng.serve()                  # until the head shuts the ring down
            import torch.distributed as dist
            dist.barrier()
            eng.channel.close()
            dist.destroy_process_group()
            rec["state"] = "stopped"
        except BaseException as e:  # noqa: BLE001 — reported by /health
            log.exception("pipeline join (%s stage %d/%d) failed: %s", name, rank, world, e)
            # a retry with a new spec must rendezvous afresh, not reuse this group: the
            # state reads "failed" only once the old group is gone
            with self.lock:
                eng = eng or self._pipe_engine
                self._pipe_engine = None
                self._teardown_idle.clear()
                rec["state"], rec["error"] = "tearing_down", str(e)
            try:
                self._abort_ring(eng)
            except Exception as e2:  # noqa: BLE001
                log.warning("pipeline teardown after a failed join: %s", e2)
            finally:
                with self.lock:
                    rec["state"] = "failed"
                    self._teardown_idle.set()

    def _abort_ring(self, eng) -> None:
        """Tear down a broken ring's transports + process group without a goodbye: the data
        plane is aborted (IPC mailboxes sticky-failed with every flag set, a direct RCCL
        communicator ncclCommAbort'ed), the compute stream is drained with a bound (the
        channel re-aborts while it waits), and the torch process group is aborted through
        the public ``ProcessGroup.abort()`` rather than destroyed (a destroy would wait on
        the dead rank). Called WITHOUT the worker lock: /health and a re-forming
        ``/load_shard`` stay responsive meanwhile."""
        import torch.distributed as dist
        ch = getattr(eng, "channel", None) if eng is not None else None
        if ch is not None:
            try:
                if ch.dead_peer is None:
                    ch.dead_peer = "ring aborted by the worker"
                ch.abort_data_plane()
                if not ch.drain(timeout_s=10.0):
                    log.warning("compute stream did not drain within 10 s after the abort")
                ch.close()
            except Exception as e:  # noqa: BLE001
                log.warning("channel teardown after a ring failure: %s", e)
        if dist.is_initialized():
            try:
                if dist.get_backend() == "nccl":
                    dist.group.WORLD.abort()
                dist.destroy_process_group()
            except Exception as e:  # noqa: BLE001
                log.warning("process group teardown after a ring failure: %s", e)

    def _pipeline_failed(self, err) -> None:
        """Head's session raised (PipelineService.on_failure): abort the ring, keep serving
        503s (the service keeps its error) until a new pipeline spec re-forms it. The abort
        runs outside the worker lock (it drains a GPU stream)."""
        log.error("pipeline %s failed: %s", getattr(self, "pipeline_model", None), err)
        with self.lock:
            eng, self._pipe_engine = self._pipe_engine, None
            rec = self.pipeline
            self._teardown_idle.clear()
            if rec is not None:
                rec["state"], rec["error"] = "tearing_down", str(err)
        try:
            self._abort_ring(eng)
            if self.device.type == "cuda":
                torch.cuda.empty_cache()
        finally:
            # "failed" (re-formable) only after the old group is destroyed: a join that
            # raced this teardown waits on _teardown_idle instead of rendezvousing under it
            with self.lock:
                if rec is not None:
                    rec["state"] = "failed"
                self._teardown_idle.set()

    def _clear_pipeline(self) -> None:
        """Forget a failed / stopped ring before joining a new one."""
        svc = getattr(self, "pipeline_service", None)
        if svc is not None:
            svc.close()
        if self._pipe_engine is not None:
            self._abort_ring(self._pipe_engine)
        self.pipeline_service = None
        self.pipeline_model = None
        self.pipeline_shards = []
        self._pipe_engine = None
        self.pipeline = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()

    def _leave_pipeline(self):
        """Rank 0: unload of the pipeline model shuts the whole ring down."""
        svc = getattr(self, "pipeline_service", None)
        eng = self._pipe_engine
        if svc is not None:
            svc.close()
        if eng is not None and eng.head is not None:
            import torch.distributed as dist
            if svc is None or svc.error is None:      # a broken ring gets no goodbye
                eng.shutdown()
                dist.barrier()
            eng.channel.close()
            dist.destroy_process_group()
        self.pipeline_service = None
        self.pipeline_model = None
        self.pipeline_shards = []
        self._pipe_engine = None
        if self.pipeline is not None:
            self.pipeline["state"] = "stopped"

    def shard_pipeline(self, name: str, shard_ids):
        """A loopback pipeline over the listed loaded shards (they must cover every layer),
        behind its own engine thread: concurrent ``shard_ids`` requests are admitted between
        ticks and batched together (the reference ran ``shard_ids[0]`` alone, one request at
        a time: worker/app.py:332-372)."""
        from ..parallel.pipeline import LocalPipeline
        key = (name, tuple(sorted(shard_ids)))
        with self.lock:
            if key in self.shard_pipes:
                return self.shard_pipes[key]
            recs = []
            for sid in sorted(shard_ids):
                if sid not in self.shards.get(name, {}):
                    raise ValueError(f"Shard {sid} of model {name} is not loaded")
                recs.append(self.shards[name][sid])
            if any(r["params"] is None for r in recs):
                raise ValueError(f"shards of {name} carry no weights (metadata-only)")
            cfg = recs[0]["cfg"]
            plans = sorted((stage_plan_from_metadata(r["metadata"]) for r in recs),
                           key=lambda p: p.start_layer)
            cover = 0
            for p in plans:
                if p.start_layer != cover:
                    break
                cover = p.end_layer
            if cover != cfg.num_layers:
                raise ValueError(f"shards {sorted(shard_ids)} of {name} cover layers [0, {cover}) "
                                 f"of {cfg.num_layers}; cannot run a partial model")
            params = {}
            for r in recs:
                params.update(r["params"])
            kw = self.engine_kwargs
            pipe = LocalPipeline(cfg, len(plans), device=self.device, max_batch=kw["max_batch"],
                                 max_model_len=kw["max_model_len"],
                                 num_blocks=kw["num_blocks"] or 4096, params=params,
                                 plans=plans, tokenizer=self.tokenizers.get(name),
                                 kv_dtype=kw.get("kv_dtype"),
                                 weight_dtype=kw.get("weight_dtype"))
            svc = EngineService(pipe, name=f"{name.replace('/', '_')}-shards")
            self.shard_pipes[key] = svc
            return svc

    def resources(self) -> dict:
        gpu_frac, extra = 0.0, {}
        if self.device.type == "cuda":
            try:
                free, total = torch.cuda.mem_get_info(self.device)
                gpu_frac = 1.0 - free / total
                extra = {"hbm_total_bytes": total, "hbm_used_bytes": total - free,
                         "gpu_name": torch.cuda.get_device_name(self.device),
                         "gpu_index": self.device.index}
                busy = gpu_busy_percent(self.device.index or 0)
                if busy is not None:
                    extra["gpu_busy"] = busy / 100.0
            except Exception:  # noqa: BLE001
                pass
        return {"cpu": psutil.cpu_percent() / 100.0,
                "memory": psutil.virtual_memory().percent / 100.0,
                "gpu": gpu_frac, "gpu_available": self.device.type == "cuda",
                "device": self.device_str, **extra}


def _shard_dtype(shard_dir: str, rank: int) -> torch.dtype:
    """Compute dtype of an exported stage = the dtype its weights were written in (the
    data plane carries activations of that dtype between stages)."""
    from safetensors import safe_open
    f = os.path.join(shard_dir, f"shard_{rank}", "model.safetensors")
    if not os.path.exists(f):
        return torch.bfloat16
    with safe_open(f, "pt") as h:
        keys = list(h.keys())
        code = h.get_slice(keys[0]).get_dtype() if keys else "BF16"   # header only
    if code == "F8_E4M3":      # FP8 weights are weight-only: the activations are bf16
        return torch.bfloat16
    return {"F32": torch.float32, "F16": torch.float16}.get(code, torch.bfloat16)


def request_params(data: dict):
    """(SamplingParams, timeout) of an /inference body: the reference's generate() call
    (worker/app.py:297-305: do_sample, T 0.8, top-k 50, top-p 0.95, max_length incl. the
    prompt) with the optional overrides this API adds."""
    max_length = int(data.get("max_length", 100))
    timeout = float(data.get("timeout", 60))
    params = SamplingParams(max_length=max_length, temperature=0.8, top_k=50, top_p=0.95,
                            timeout_s=timeout)
    for k in ("temperature", "top_k", "top_p", "seed", "max_new_tokens"):
        if k in data:
            setattr(params, k, data[k])
    return params, timeout


def success_body(out, t0: float) -> dict:
    return {"status": "success", "result": out.resolve_text(), "execution_time": time.time() - t0,
            "output_tokens": len(out.output_ids), "finish_reason": out.finish_reason}


def create_worker_app(settings: Optional[Settings] = None, device: Optional[str] = None,
                      engine_kwargs: Optional[dict] = None, state: Optional[WorkerState] = None):
    settings = settings or get_settings()
    st = state or WorkerState(settings, device, engine_kwargs)
    app = Flask(__name__)
    app.extensions["dli_worker"] = st

    def require_auth(f):
        @wraps(f)
        def wrapped(*a, **kw):
            if settings.auth_enabled:
                if request.headers.get("Authorization") != f"Bearer {settings.auth_key}":
                    return jsonify({"status": "error", "message": "Unauthorized access"}), 401
            return f(*a, **kw)
        return wrapped

    @app.get("/health")
    @require_auth
    def health():
        try:
            faults.check("worker.health")
        except faults.InjectedFault as e:
            return jsonify({"status": "error", "message": str(e)}), 503
        psvc = getattr(st, "pipeline_service", None)
        if psvc is not None and getattr(psvc, "error", None) is not None:   # a stage died
            return jsonify({"status": "error",
                            "message": f"pipeline failed: {psvc.error}"}), 503
        shard_info = [{"model_name": m, "shard_id": sid, "path": r["path"],
                       "metadata": r["metadata"]}
                      for m, sh in st.shards.items() for sid, r in sh.items()]
        if os.environ.get("DLI_REPORT_PIPELINE_SHARDS", "1") == "1":
            # a ring's head reports every stage as its shard (the master routes the model
            # here); DP replicas of one model run with 0, as plain nodes the dispatcher
            # balances (the reference's ModelShard rows are unique per (model, shard))
            shard_info += getattr(st, "pipeline_shards", None) or []
        extra = {"pipeline": st.pipeline} if st.pipeline is not None else {}
        if st.data_plane is not None:
            extra["data_plane"] = st.data_plane
        return jsonify({"status": "healthy", "resources": st.resources(), **extra,
                        "loaded_models": list(st.services.keys()),
                        "loaded_tokenizers": list(st.tokenizers.keys()),
                        "loaded_shards": shard_info})

    @app.post("/load_model")
    @require_auth
    def load_model():
        data = request.get_json(silent=True) or {}
        name = data.get("model_name")
        if not name:
            return jsonify({"status": "error", "message": "Model name is required"}), 400
        try:
            fresh = st.load_model(name)
        except Exception as e:  # noqa: BLE001
            return jsonify({"status": "error", "message": f"Failed to load model: {e}"}), 500
        if not fresh:
            return jsonify({"status": "success", "message": f"Model {name} is already loaded"})
        return jsonify({"status": "success",
                        "message": f"Model {name} loaded successfully on {st.device_str}"})

    @app.post("/load_shard")
    @require_auth
    def load_shard_ep():
        data = request.get_json(silent=True) or {}
        name, sid, path = data.get("model_name"), data.get("shard_id"), data.get("shard_path")
        if not name or sid is None or not path:
            return jsonify({"status": "error",
                            "message": "Model name, shard ID, and shard path are required"}), 400
        try:
            if isinstance(data.get("pipeline"), dict):
                fresh = st.join_pipeline(name, int(sid), str(path), data["pipeline"])
                if fresh:
                    return jsonify({"status": "success",
                                    "message": f"Shard {sid} of model {name} is joining the "
                                               f"pipeline", "pipeline": st.pipeline})
            else:
                fresh = st.load_shard(name, int(sid), str(path))
        except Exception as e:  # noqa: BLE001
            return jsonify({"status": "error", "message": f"Failed to load shard: {e}"}), 500
        if not fresh:
            return jsonify({"status": "success",
                            "message": f"Shard {sid} of model {name} is already loaded"})
        return jsonify({"status": "success",
                        "message": f"Shard {sid} of model {name} loaded successfully"})

    @app.post("/unload_model")
    @require_auth
    def unload_model():
        data = request.get_json(silent=True) or {}
        name = data.get("model_name")
        if not name:
            return jsonify({"status": "error", "message": "Model name is required"}), 400
        try:
            st.unload_model(name)
        except Exception as e:  # noqa: BLE001
            return jsonify({"status": "error", "message": f"Failed to unload model: {e}"}), 500
        return jsonify({"status": "success", "message": f"Model {name} unloaded successfully"})

    @app.post("/inference")
    @require_auth
    def run_inference():
        data = request.get_json(silent=True) or {}
        name, prompt = data.get("model_name"), data.get("prompt")
        if not name or not prompt:
            return jsonify({"status": "error",
                            "message": "Model name and prompt are required"}), 400
        shard_ids = data.get("shard_ids")
        t0 = time.time()
        params, timeout = request_params(data)
        try:
            faults.check("worker.inference")
            svc = getattr(st, "pipeline_service", None)
            if svc is not None and name == getattr(st, "pipeline_model", None):
                # pipeline head (serve-pipeline / one DP replica of serve-cluster): every
                # stage of this model runs on this rank's pipeline, with or without shard_ids
                if getattr(svc, "error", None) is not None:   # broken ring: next replica retries
                    return jsonify({"status": "error",
                                    "message": f"pipeline failed: {svc.error}"}), 503
                try:
                    out = svc.generate(prompt, params, timeout=timeout + 30)
                except PipelineFailed as e:
                    return jsonify({"status": "error", "message": str(e)}), 503
            elif (st.pipeline is not None and st.pipeline["model_name"] == name
                  and st.pipeline["rank"] != 0):
                return jsonify({"status": "error",
                                "message": f"Inference failed: this node is stage "
                                           f"{st.pipeline['rank']} of the {name} pipeline; "
                                           f"requests enter at its stage-0 node"}), 409
            elif shard_ids:
                svc = st.shard_pipeline(name, [int(s) for s in shard_ids])
                out = svc.generate(prompt, params, timeout=timeout + 30)
            else:
                if name not in st.services:
                    try:
                        st.load_model(name)
                    except Exception as e:  # noqa: BLE001
                        return jsonify({"status": "error",
                                        "message": f"Failed to load model: {e}"}), 500
                out = st.services[name].generate(prompt, params, timeout=timeout + 30)
            if out.finish_reason == "timeout":
                raise TimeoutError("Inference generation timed out")
            return jsonify(success_body(out, t0))
        except TimeoutError as e:
            return jsonify({"status": "error", "message": str(e)}), 408
        except Exception as e:  # noqa: BLE001
            return jsonify({"status": "error", "message": f"Inference failed: {e}"}), 500

    @app.post("/ssh_setup")
    @require_auth
    def ssh_setup():
        data = request.get_json(silent=True) or {}
        host, port = data.get("host"), int(data.get("port", 22))
        user, pw, key = data.get("username"), data.get("password"), data.get("key_path")
        if not host or not (pw or key) or not user:
            return jsonify({"status": "error", "message": "Host, username, and either password "
                            "or key_path are required"}), 400
        try:
            try:
                import paramiko  # not installed in this image
            except ImportError:
                paramiko = None
            if paramiko is not None:
                c = paramiko.SSHClient()
                c.set_missing_host_key_policy(paramiko.AutoAddPolicy())
                if key:
                    c.connect(hostname=host, port=port, username=user,
                              pkey=paramiko.RSAKey.from_private_key_file(key))
                else:
                    c.connect(hostname=host, port=port, username=user, password=pw)
                c.close()
                return jsonify({"status": "success",
                                "message": f"SSH connection to {host} established successfully"})
            with socket.create_connection((host, port), timeout=5) as s:
                banner = s.recv(64).decode(errors="replace").strip()
            return jsonify({"status": "success",
                            "message": f"SSH connection to {host} established successfully "
                                       f"(transport probe only; paramiko unavailable, "
                                       f"credentials not verified; banner: {banner!r})"})
        except Exception as e:  # noqa: BLE001
            return jsonify({"status": "error", "message": f"SSH connection failed: {e}"}), 500

    @app.get("/metrics")
    @require_auth
    def metrics():
        out = {name: svc.stats() for name, svc in st.services.items()}
        if getattr(st, "pipeline_service", None) is not None:
            out[st.pipeline_model] = st.pipeline_service.stats()
        body = {"engines": out, "resources": st.resources()}
        if st.data_plane is not None:
            body["data_plane"] = st.data_plane
        return jsonify(body)

    return app


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser("dli serve-worker")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=5000)
    ap.add_argument("--gpu", type=int, default=None, help="GPU index (implies USE_GPU=1)")
    ap.add_argument("--preload", default="", help="comma-separated models to load at start")
    ap.add_argument("--max-batch", type=int, default=None)
    ap.add_argument("--kv-dtype", default=None, choices=["bf16", "fp8"],
                    help="element type of the paged KV cache (default: KV_CACHE_DTYPE, bf16)")
    ap.add_argument("--weight-dtype", default=None, choices=["bf16", "fp8"],
                    help="fp8: quantise the llama-family projections and experts to block-scaled "
                         "FP8 "
                         "(default: WEIGHT_DTYPE, or the checkpoint's own)")
    ap.add_argument("--server", default="werkzeug", choices=["werkzeug", "uvicorn", "aiohttp"],
                    help="uvicorn: ASGI front (worker/asgi.py: /inference as a coroutine per "
                         "request) over the same Flask app; aiohttp: the same ASGI front on "
                         "aiohttp's C HTTP parser (utils/aioserve.py)")
    a = ap.parse_args(argv)
    setup_logging(f"worker{a.port}")
    s = get_settings()
    dev = None
    if a.gpu is not None:
        s.use_gpu = True
        dev = f"cuda:{a.gpu}"
        if torch.cuda.is_available():
            # every GPU of the node is visible (serve-node): make this worker's GPU the
            # current one, so nothing lands on device 0 by default
            torch.cuda.set_device(a.gpu)
    kw = {"max_batch": a.max_batch} if a.max_batch else None
    if a.kv_dtype:
        s.kv_cache_dtype = a.kv_dtype
        kw = dict(kw or {}, kv_dtype=a.kv_dtype)
    if a.weight_dtype:
        s.weight_dtype = a.weight_dtype
        kw = dict(kw or {}, weight_dtype=a.weight_dtype)
    app = create_worker_app(s, dev, kw)
    for m in [m for m in a.preload.split(",") if m]:
        app.extensions["dli_worker"].load_model(m)
    if a.server == "aiohttp":
        from ..utils.aioserve import run_asgi
        from .asgi import create_asgi_app
        run_asgi(create_asgi_app(app), host=a.host, port=a.port)
        return
    if a.server == "uvicorn":
        import uvicorn

        from .asgi import create_asgi_app
        uvicorn.run(create_asgi_app(app), host=a.host, port=a.port, log_level="warning",
                    timeout_keep_alive=75, backlog=4096)
        return
    app.run(host=a.host, port=a.port, threaded=True)


if __name__ == "__main__":
    main()
