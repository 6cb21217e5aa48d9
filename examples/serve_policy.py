"""Minimal policy-serving endpoint on MI355X.

Serves the flagship MLP policy's actions over HTTP (FastAPI/uvicorn,
both in the image): requests are micro-batched and run through
`ESEngine.act`, which normalises the observations with the trained
engine's running statistics, as the rollout kernels do, and evaluates
them with the MFMA `mlp_policy_forward` kernel.  The served action is
the one the training loop would have taken in that state.

Run (on a GPU node):  python examples/serve_policy.py --port 8080
Query:                curl -X POST localhost:8080/act \
                        -H 'content-type: application/json' \
                        -d '{"obs": [[0.1, -0.2, 0.05, 0.0]]}'

A request whose `obs` is not a list of rows of 4 numbers is answered
with 422 and never reaches the device.
"""

import os as _os
import sys as _sys

_REPO_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _REPO_ROOT not in _sys.path:
    _sys.path.insert(0, _REPO_ROOT)


import argparse

OBS_DIM = 4
MAX_BATCH = 65536  # rows per request


def parse_obs(obs):
    """The request's ``obs`` as a contiguous fp32 CPU tensor ``[n][4]``;
    ValueError for anything else (ragged or non-numeric rows, a flat list,
    a row that is not 4 wide, more than MAX_BATCH rows).  ``[]`` is an
    empty batch."""
    import torch

    if not isinstance(obs, list):
        raise ValueError("obs must be a list of rows of %d numbers" % OBS_DIM)
    if len(obs) > MAX_BATCH:
        raise ValueError("at most %d rows per request, got %d"
                         % (MAX_BATCH, len(obs)))
    if not obs:
        return torch.empty(0, OBS_DIM, dtype=torch.float32)
    try:
        x = torch.tensor(obs, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError) as exc:
        raise ValueError("obs is not a rectangular list of numbers: %s"
                         % exc) from None
    if x.dim() != 2 or x.shape[1] != OBS_DIM:
        raise ValueError("obs must be [n][%d], got shape %s"
                         % (OBS_DIM, list(x.shape)))
    return x.contiguous()


def build_app(checkpoint=None):
    import torch
    from fastapi import FastAPI, HTTPException
    from pydantic import BaseModel

    from fiber_amd.es import ESConfig, ESEngine

    device = torch.device("cuda", 0)
    engine = ESEngine(ESConfig(), ctx=None, device=device)
    if checkpoint:
        engine.load(checkpoint)

    class ActRequest(BaseModel):
        obs: list  # [[obs_dim floats], ...]

    app = FastAPI(title="fiber_amd policy server")

    @app.post("/act")
    def act(req: ActRequest):
        try:
            x = parse_obs(req.obs)
        except ValueError as exc:
            raise HTTPException(status_code=422, detail=str(exc))
        actions, logits = engine.act(x.to(device), return_logits=True)
        return {
            "actions": actions.tolist(),
            "logits": logits.tolist(),
        }

    @app.get("/healthz")
    def healthz():
        return {"ok": True, "device": torch.cuda.get_device_name(0)}

    return app


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--port", type=int, default=8080)
    parser.add_argument("--checkpoint", default=None)
    args = parser.parse_args()
    import uvicorn

    uvicorn.run(build_app(args.checkpoint), host="127.0.0.1",
                port=args.port)


if __name__ == "__main__":
    main()
