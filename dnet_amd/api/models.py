"""API DTOs: OpenAI-compatible chat types + topology/load requests.

Reference counterpart: src/dnet/api/models.py.
"""
from __future__ import annotations

import time
import uuid
from typing import Any, Optional

from pydantic import BaseModel, Field, field_validator, model_serializer


class ChatMessage(BaseModel):
    role: str
    content: Optional[str] = None
    name: Optional[str] = None


class ChatRequestModel(BaseModel):
    model: str
    messages: list[ChatMessage]
    max_tokens: Optional[int] = None
    max_completion_tokens: Optional[int] = None
    temperature: float = 0.0
    seed: int | None = None
    top_p: float = 1.0
    top_k: int = 0
    min_p: float = 0.0
    # HF/vLLM multiplicative penalty (> 0) and the two OpenAI additive
    # ones (range [-2, 2]); out of range is a 422
    repetition_penalty: float = Field(default=1.0, gt=0.0)
    presence_penalty: float = Field(default=0.0, ge=-2.0, le=2.0)
    frequency_penalty: float = Field(default=0.0, ge=-2.0, le=2.0)
    # OpenAI logit_bias: token id (as a string key, below 2^31) -> bias in
    # [-100, 100], at most 300 entries; anything else is a 422
    logit_bias: Optional[dict[str, float]] = None
    stream: bool = False
    stop: Optional[list[str] | str] = None
    logprobs: bool = False
    top_logprobs: int = 0
    profile: bool = False            # emit metrics in the final chunk
    n: int = 1
    # false: this request neither reads nor feeds the shard's prompt-prefix
    # KV cache (no effect when the cache is off)
    cache_prompt: bool = True

    @field_validator("logit_bias")
    @classmethod
    def _check_logit_bias(cls, v):
        if v is None:
            return v
        if len(v) > 300:
            raise ValueError("logit_bias: at most 300 entries")
        for k, b in v.items():
            # a token id: ASCII digits, below 2^31 (no vocabulary is larger,
            # and the id must fit the int64 words the runtime broadcasts)
            if not (k.isascii() and k.isdigit() and len(k) <= 10
                    and int(k) < 2 ** 31):
                raise ValueError(
                    f"logit_bias: key {k!r} is not a token id "
                    "(a non-negative integer below 2^31)")
            if not -100.0 <= b <= 100.0:
                raise ValueError(
                    f"logit_bias: value {b!r} outside [-100, 100]")
        return v

    @property
    def effective_max_tokens(self) -> int:
        return self.max_completion_tokens or self.max_tokens or 128


class UsageModel(BaseModel):
    prompt_tokens: int = 0
    completion_tokens: int = 0
    total_tokens: int = 0
    # OpenAI shape {"cached_tokens": n}; set only when the shard reported a
    # prefix-cache lookup for the request
    prompt_tokens_details: Optional[dict] = None

    @model_serializer(mode="wrap")
    def _drop_unset_details(self, handler):
        # the key is absent, not null, when nothing was reported: responses
        # stay byte-identical to a server without a prefix cache
        d = handler(self)
        if d.get("prompt_tokens_details") is None:
            d.pop("prompt_tokens_details", None)
        return d


class ChoiceDelta(BaseModel):
    role: Optional[str] = None
    content: Optional[str] = None


class StreamChoice(BaseModel):
    index: int = 0
    delta: ChoiceDelta = Field(default_factory=ChoiceDelta)
    finish_reason: Optional[str] = None
    logprobs: Optional[dict] = None


class ChatChunkModel(BaseModel):
    id: str
    object: str = "chat.completion.chunk"
    created: int = Field(default_factory=lambda: int(time.time()))
    model: str = ""
    choices: list[StreamChoice] = Field(default_factory=list)
    usage: Optional[UsageModel] = None
    metrics: Optional[dict] = None


class ChoiceMessage(BaseModel):
    role: str = "assistant"
    content: str = ""


class Choice(BaseModel):
    index: int = 0
    message: ChoiceMessage = Field(default_factory=ChoiceMessage)
    finish_reason: str = "stop"
    logprobs: Optional[dict] = None


class ChatResponseModel(BaseModel):
    id: str
    object: str = "chat.completion"
    created: int = Field(default_factory=lambda: int(time.time()))
    model: str = ""
    choices: list[Choice] = Field(default_factory=list)
    usage: UsageModel = Field(default_factory=UsageModel)
    metrics: Optional[dict] = None


def new_nonce() -> str:
    return f"chatcmpl-{uuid.uuid4()}"


class ModelInfo(BaseModel):
    id: str
    object: str = "model"
    created: int = 0
    owned_by: str = "dnet_amd"


class ModelListResponse(BaseModel):
    object: str = "list"
    data: list[ModelInfo] = Field(default_factory=list)


class PrepareTopologyRequest(BaseModel):
    model: str
    seq_len: int = 512
    batch_size: int = 1
    kv_bits: int = 16
    quant: str = ""


class ManualAssignment(BaseModel):
    instance: str
    layers: list[int]


class PrepareTopologyManualRequest(BaseModel):
    model: str
    assignments: list[ManualAssignment]
    kv_bits: int = 16
    quant: str = ""


class APILoadModelRequest(BaseModel):
    model: str
    quant: str = ""
    # >1 = slot-scheduled continuous batching (the production serving
    # mode: concurrent requests each own a KV slot; per-slot sampling,
    # seeds, logprobs and hipGraph decode all supported). 1 = serial.
    max_batch: int = 8
    max_seq: int = 4096
    warmup: bool = False
    # prompt-prefix KV cache entries per shard (0 = off; needs
    # max_batch > 1 on a single-rank ring)
    prefix_cache: int = 0
