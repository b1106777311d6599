"""Stream orchestrator with the surface AND the signatures of the reference's `LiveCCDemoInfer` (ref demo/infer.py:25-310),
driving the native model instead of HF, so that the L5 callers run unmodified given decoded frames:

    infer = LiveCCDemoInfer(model_path=..., device='cuda:0')                          # ref demo/cli.py:9
    state = {'video_path': path}; state['video_timestamp'] = t
    for (t0, t1), response, state in infer.live_cc(message=query, state=state, max_pixels=..., repetition_penalty=1.05,
                                                   streaming_eos_base_threshold=0.0, streaming_eos_threshold_step=0): ...
    responses = infer.live_cc_once_for_evaluation(query=..., video=video, video_start=b, video_end=e,
                                                  max_new_tokens=32, repetition_penalty=1.15)   # ref distributed_generate_livecc.py:84
    response, state = infer.video_qa(message, history, state)                         # ref demo/app.py

Video DECODING stays external (decord is a C++ dependency of the reference): `video_path` / `video` name a
`livecc_amd.video.DecodedVideo` (uint8 frames + pts) registered with `video.register_video`, produced by a loader installed with
`video.set_video_loader`, or passed directly.  Everything after the decoder runs here: frame selection
(`video.read_video_decord_plus`, `resize.select_clip_frames`), the pixel-budget policy, the antialias-bicubic resize on the GPU,
the chunking 6/2/2..., the turn text, and `generate` on the native engine.

Text: with tokenizer files (a checkpoint directory, or a `text.TextFrontEnd` passed in) the turns are built from real strings
exactly as the reference does -- chat template, 'Time=a-bs' prefix, query appended on the first turn or when it changes,
'<|im_end|>\\n' glue, `processor.decode` of the answer (ref demo/infer.py:134-157, 175); without them the turn ids are synthetic
(`protocol.TurnBuilder`; benchmarks and shape tests) and "responses" are the generated ids joined by spaces.

The clip-level entry points (`live_cc_clip`, `video_qa_clip`) take an already fetched + resized uint8 clip; the multi-stream
server and the benchmarks use them.
"""
from __future__ import annotations

import contextlib
from typing import Callable, List, Optional

import numpy as np
import torch

from . import protocol
from . import video as V
from .modeling import LiveCCForConditionalGeneration


class ThresholdLogitsProcessor:
    """ref demo/infer.py:10-23.  Executed natively inside the fused sampler kernel; this object only carries the
    parameters (and the `count` the reference keeps)."""

    def __init__(self, token_id: int, base_threshold: float, step: float):
        self.token_id, self.base_threshold, self.step, self.count = token_id, base_threshold, step, 0


def _hw(clip: torch.Tensor, layout: str):
    return (clip.shape[2], clip.shape[3]) if layout == "TCHW" else (clip.shape[1], clip.shape[2])


class LiveCCDemoInfer:
    MAX_CACHED_READERS = 8     # decoded-video readers kept by live_cc (the reference never evicts; a long-running server must)
    VIDEO_PLAY_END = object()
    VIDEO_PLAY_CONTINUE = object()
    fps = protocol.FPS
    initial_fps_frames = protocol.INITIAL_FPS_FRAMES
    streaming_fps_frames = protocol.STREAMING_FPS_FRAMES
    initial_time_interval = protocol.INITIAL_TIME_INTERVAL
    streaming_time_interval = protocol.STREAMING_TIME_INTERVAL
    frame_time_interval = protocol.FRAME_TIME_INTERVAL

    def __init__(self, model_path: str = None, device: str = None, model: LiveCCForConditionalGeneration = None,
                 turn_builder: Optional[protocol.TurnBuilder] = None, decode: Optional[Callable[[List[int]], str]] = None,
                 streaming_eos_token_id: Optional[int] = None, text=None, **model_kw):
        """ref demo/infer.py:35-59.  `text`: a `text.TextFrontEnd` (real tokenizer); with `model_path` it is created from the
        checkpoint directory's tokenizer files when they exist.  `model_kw` (max_streams, max_kv_len, llm_weights ...) goes to
        `from_pretrained`."""
        if model is None:
            device = device or "cuda"
            model = LiveCCForConditionalGeneration.from_pretrained(model_path, torch_dtype="auto", device_map=device, **model_kw)
        self.model = model
        self.cfg = model.cfg
        if text is None and model_path is not None:
            import os
            if any(os.path.exists(os.path.join(model_path, f)) for f in ("tokenizer.json", "vocab.json", "tokenizer_config.json")):
                from .text import TextFrontEnd
                text = TextFrontEnd(model_path, self.cfg)
        self.text = text
        self.turn_builder = turn_builder or protocol.TurnBuilder(self.cfg)
        if text is not None:
            self.decode = decode or (lambda ids: text.decode(ids, skip_special_tokens=True))
            self.streaming_eos_token_id = text.streaming_eos_token_id if streaming_eos_token_id is None else streaming_eos_token_id
            self.system_prompt_offset = text.system_prompt_offset
        else:
            self.decode = decode or (lambda ids: " ".join(str(i) for i in ids))
            # ref infer.py:49: tokenizer(' ...').input_ids[-1]; without tokenizer files the caller supplies it
            self.streaming_eos_token_id = streaming_eos_token_id
            self.system_prompt_offset = None
        self._cached_video_readers_with_hw = {}
        self.last_generated: list = []      # per generate call of the most recent flows: span, new prompt ids, generated ids

    def close_video(self, video_path) -> None:
        """Drop the cached reader of a finished video (path or DecodedVideo object) so that its frames can be freed."""
        self._cached_video_readers_with_hw.pop(video_path if isinstance(video_path, str) else id(video_path), None)

    # --------------------------------------------------------------------------------------------------------------
    # one generate call per chunk (ref demo/infer.py:132-180, step 5)
    # --------------------------------------------------------------------------------------------------------------
    def _turn(self, frames, frames_layout, start, stop, state, message, default_query, do_sample, repetition_penalty,
              streaming_eos_base_threshold, streaming_eos_threshold_step, max_new_tokens, force_length, gen_kw, kv_window=None):
        turn = state.get("turn_index", 0)
        grid = protocol.grid_of(frames.shape[0], *_hw(frames, frames_layout), self.cfg)
        past_ids = state.get("past_ids")
        if self.text is not None:
            if not message and not state.get("message"):
                message = default_query                       # ref infer.py:141-143
            query = None
            if message and state.get("message") != message:   # ref infer.py:144-146
                query = message
                state["message"] = message
            new_ids = self.text.turn_ids(start, stop, grid, query, continuing=past_ids is not None)
        else:
            new_ids = self.turn_builder.turn_ids(turn, protocol.num_video_tokens(grid, self.cfg))
        if kv_window in ("slide", "slide_rebase") and past_ids is not None:
            past_ids = self._slide(state, past_ids, len(new_ids), rebase=kv_window == "slide_rebase")
        ids = new_ids if past_ids is None else np.concatenate([past_ids, new_ids])
        procs = None
        if streaming_eos_base_threshold is not None and self.streaming_eos_token_id is not None:
            procs = [ThresholdLogitsProcessor(self.streaming_eos_token_id, streaming_eos_base_threshold,
                                              streaming_eos_threshold_step or 0.0)]
        out = self.model.generate(
            input_ids=torch.from_numpy(ids).view(1, -1), frames=frames, frames_layout=frames_layout,
            past_key_values=state.get("past_key_values"), return_dict_in_generate=True, do_sample=do_sample,
            repetition_penalty=repetition_penalty, logits_processor=procs, max_new_tokens=max_new_tokens,
            min_new_tokens=max_new_tokens if force_length else None, pad_token_id=self.cfg.eos_token_id, **gen_kw)
        seq = out.sequences[0].cpu().numpy()
        state["past_key_values"] = out.past_key_values
        state["past_ids"] = seq[:-1]                      # ref infer.py:174
        state["turn_index"] = turn + 1
        if kv_window in ("slide", "slide_rebase"):
            spans = state.get("turn_spans") or []
            begin = spans[-1][1] if spans else 0           # (a state that did not slide before: everything cached so far is the head)
            state["turn_spans"] = spans + [(begin, len(seq) - 1)]
        new_tokens = seq[len(ids):].tolist()
        self.last_generated.append(dict(span=(start, stop), prompt_ids=new_ids, tokens=new_tokens))   # diagnostics / parity tests
        return self.decode([t for t in new_tokens if t not in self.model.eos_token_ids])

    def _slide(self, state, past_ids, need, rebase=False):
        """kv_window="slide" / "slide_rebase": when the next turn would not fit the KV slot, the oldest whole turns after the head leave
        the cache (protocol.plan_eviction + StreamState.evict, with rebase=True for "slide_rebase") and `past_ids`; returns the
        (possibly shorter) past_ids."""
        eng = self.model.engine
        cap = eng.max_kv_len - eng.max_history
        if len(past_ids) + need <= cap:
            return past_ids
        spans = state.get("turn_spans") or []
        if not spans or spans[-1][1] != len(past_ids):
            return past_ids                               # no usable turn table: the engine's own capacity error applies, as without a window
        plan = protocol.plan_eviction(spans, len(past_ids), need, cap)
        if plan is None:
            return past_ids
        first, n, k = plan
        kept = np.concatenate([past_ids[:first], past_ids[first + n:]])
        if rebase:
            state["past_key_values"].evict(first, n, kept, rebase=True)
        else:
            state["past_key_values"].evict(first, n, kept)
        state["past_ids"] = kept
        state["turn_spans"] = spans[:1] + [(b - n, e - n) for b, e in spans[1 + k:]]
        state["evictions"] = state.get("evictions", 0) + 1
        return kept

    # --------------------------------------------------------------------------------------------------------------
    # live_cc: the reference's signature (ref demo/infer.py:61-180)
    # --------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def live_cc(self, message: str, state: dict, max_pixels: int = 384 * 28 * 28, default_query: str = "Please describe the video.",
                do_sample: bool = True, repetition_penalty: float = 1.05, streaming_eos_base_threshold: float = None,
                streaming_eos_threshold_step: float = None, hf_spaces: bool = False, kv_window: str = None, **kwargs):
        """state keys as in the reference: video_path, video_timestamp, last_timestamp, last_video_pts_index, video_pts,
        past_ids, past_key_values, message, video_end.  Extra keyword arguments: max_new_tokens (16), force_length,
        and sampling parameters (top_k / top_p / temperature / seed) forwarded to `generate`.  Yields
        ((start, stop), response, state).
        kv_window: None = the reference's behaviour (the cache grows until the engine refuses the prefill); "slide" = when the next
        turn would not fit the KV slot, the oldest whole turns after the first one are evicted on the device (down to half the
        window) and the stream continues; the turn table lives in state['turn_spans'], the count in state['evictions'];
        "slide_rebase" = "slide", and the kept keys are rotated back by the evicted row count (StreamState.evict(rebase=True)), so the
        rope positions stay inside the KV slot as well: the next position never passes max_kv_len + the first turn's rope_delta."""
        if kv_window not in (None, "slide", "slide_rebase"):
            raise ValueError(f"kv_window must be None, 'slide' or 'slide_rebase', got {kv_window!r}")
        max_new_tokens = int(kwargs.pop("max_new_tokens", 16))
        force_length = bool(kwargs.pop("force_length", False))
        # 1. preparation: video reader and last processing info (ref :86-104)
        video_timestamp, last_timestamp = state.get("video_timestamp", 0), state.get("last_timestamp", -1 / self.fps)
        video_path = state.get("video_path", None)
        if video_path is None or (isinstance(video_path, str) and not video_path):
            return
        key = video_path if isinstance(video_path, str) else id(video_path)
        if key not in self._cached_video_readers_with_hw:
            self._cached_video_readers_with_hw[key] = V.get_smart_resized_video_reader(video_path, max_pixels)
            while len(self._cached_video_readers_with_hw) > self.MAX_CACHED_READERS:       # oldest first (dict order)
                self._cached_video_readers_with_hw.pop(next(iter(self._cached_video_readers_with_hw)))
        if state.get("video_pts") is None:
            # the reference fills these only when it opens the reader (:91-95), so a second state over an already cached video
            # silently yields nothing there; here every new state starts from the cached reader
            state["video_pts"] = self._cached_video_readers_with_hw[key][0].pts
            state["last_video_pts_index"] = -1
        video_pts = state.get("video_pts", None)
        if video_pts is None:
            return
        video_timestamp = min(video_timestamp, video_pts[-1])
        if last_timestamp + self.frame_time_interval > video_pts[-1]:
            state["video_end"] = True
            return
        reader, resized_height, resized_width = self._cached_video_readers_with_hw[key]
        last_video_pts_index = state["last_video_pts_index"]
        # 2. which frames will be processed (ref :106-111)
        initialized = last_timestamp >= 0
        if not initialized:
            video_timestamp = max(video_timestamp, self.initial_time_interval)
        if video_timestamp <= last_timestamp + self.frame_time_interval:
            return
        timestamps = torch.arange(last_timestamp + self.frame_time_interval, video_timestamp, self.frame_time_interval).tolist()
        # 3. fetch frames at the required timestamps, resized on the GPU (ref :113-118)
        # Only the frames that are due travel to HBM (the reference fetches exactly these with decord's get_batch, ref
        # video_process_patch.py:146): the frame indices are chosen on the host, `reader.get_batch` uploads them (a decoded video
        # that already lives on the GPU is indexed in place) and the resize runs on the GPU.  A 5-minute 1080p30 video is ~56 GB of
        # uint8 frames -- it is never made resident as a whole.
        from . import resize as R
        clip, clip_timestamps, clip_idxs = R.get_smart_resized_clip(reader, resized_height, resized_width, timestamps, video_pts,
                                                                   last_video_pts_index + 1, reader.layout, device=self.model.device)
        if len(clip_idxs) == 0:
            return
        state["last_video_pts_index"] = clip_idxs[-1]
        state["last_timestamp"] = clip_timestamps[-1]
        # 4. interleave: first chunk 6 frames, then chunks of 2 (ref :120-129); 5. one generate per chunk (ref :131-180)
        for a, b in protocol.split_clip(clip.shape[0], initialized):
            ts = clip_timestamps[a:b]
            start, stop = ts[0], ts[-1] + self.frame_time_interval
            response = self._turn(clip[a:b], "TCHW", start, stop, state, message, default_query, do_sample, repetition_penalty,
                                  streaming_eos_base_threshold, streaming_eos_threshold_step, max_new_tokens, force_length, kwargs, kv_window)
            if hf_spaces:   # ref :176-178: the caller gets a light copy without the device-side state
                yield (start, stop), response, {k: v for k, v in state.items() if k not in ("past_ids", "past_key_values")}
            else:
                yield (start, stop), response, state

    @torch.inference_mode()
    def live_cc_clip(self, clip: torch.Tensor, state: dict, frames_layout: str = "TCHW", do_sample: bool = False,
                     repetition_penalty: float = 1.05, streaming_eos_base_threshold: float = None,
                     streaming_eos_threshold_step: float = None, max_new_tokens: int = 16, force_length: bool = False,
                     message: Optional[str] = None, default_query: str = "Please describe the video.", hf_spaces: bool = False,
                     **gen_kw):
        """Steps 4-5 of `live_cc` on frames that are already fetched and resized (`clip` uint8 [T,3,H,W] or THWC): the frames
        continue the stream at state['last_timestamp'] + 0.5 s.  Yields ((start, stop), text, state) per chunk."""
        initialized = state.get("last_timestamp", -1.0) >= 0
        t0 = state.get("last_timestamp", -self.frame_time_interval) + self.frame_time_interval
        for a, b in protocol.split_clip(clip.shape[0], initialized):
            start = t0 + a * self.frame_time_interval
            stop = t0 + b * self.frame_time_interval
            text_out = self._turn(clip[a:b], frames_layout, start, stop, state, message, default_query, do_sample, repetition_penalty,
                                  streaming_eos_base_threshold, streaming_eos_threshold_step, max_new_tokens, force_length, gen_kw)
            state["last_timestamp"] = stop - self.frame_time_interval
            if hf_spaces:
                yield (start, stop), text_out, {k: v for k, v in state.items() if k not in ("past_ids", "past_key_values")}
            else:
                yield (start, stop), text_out, state

    # --------------------------------------------------------------------------------------------------------------
    # video_qa (ref demo/infer.py:182-242)
    # --------------------------------------------------------------------------------------------------------------
    def _fetch_video(self, video):
        """`qwen_vl_utils.process_vision_info` -> `fetch_video` with the reference's 'decord+' backend (ref
        video_process_patch.py:85-86): `_read_video_decord_plus(ele)` (smart_nframes + linspace), then the per-nframes pixel
        budget + smart_resize + antialias bicubic resize -- the same arithmetic as `_spatial_resize_video`."""
        clip, _ = V.read_video_decord_plus({"video": video}, device=self.model.device)
        return V.spatial_resize_video(clip, device=self.model.device)

    @torch.inference_mode()
    def video_qa(self, message, history: list, state: dict, do_sample: bool = False, repetition_penalty: float = 1.05,
                 hf_spaces: bool = False, **kwargs):
        """The reference's signature.  First turn (no `past_ids`): the whole video named by state['video_path'] in ONE prefill
        (up to 480 frames / 24k visual tokens) + `message`; later turns: text only on the carried KV.  `hf_spaces`: stateless --
        the conversation is rebuilt from `history` ([{'role','content'}...]) and nothing is kept.  Returns (response, state).
        `message` is the query string (tokenizer mode) or a synthetic query length (int)."""
        max_new_tokens = int(kwargs.pop("max_new_tokens", 512))
        force_length = bool(kwargs.pop("force_length", False))
        video_path = state.get("video_path", None)
        past_ids = state.get("past_ids", None)
        use_video = video_path is not None and (hf_spaces or past_ids is None)      # "only use once" (ref :206, 214)
        if hf_spaces:
            past_ids = None
            old = state.get("past_key_values")
            if old is not None:
                old.release()
                state["past_key_values"] = None
        clip = self._fetch_video(video_path) if use_video else None
        grid = protocol.grid_of(clip.shape[0], clip.shape[2], clip.shape[3], self.cfg) if clip is not None else None
        if isinstance(message, str):
            if self.text is None:
                raise ValueError("a query string needs tokenizer files (pass text=TextFrontEnd(...) or a checkpoint directory)")
            conversation = []
            video_pending = clip is not None
            if hf_spaces:                                                            # ref :202-210
                for past_message in history or []:
                    content = [{"type": "text", "text": past_message["content"]}]
                    if video_pending:
                        content.insert(0, {"type": "video", "video": None})
                        video_pending = False
                    conversation.append({"role": past_message["role"], "content": content})
            content = [{"type": "text", "text": message}]
            if video_pending:
                content.insert(0, {"type": "video", "video": None})
            conversation.append({"role": "user", "content": content})
            text = self.text.apply_chat_template(conversation, add_generation_prompt=True)
            if past_ids is not None:
                text = "<|im_end|>\n" + text[self.text.system_prompt_offset:]        # ref :218-219
            new_ids = self.text.encode(text, [grid] if grid is not None else [])
        else:
            self.turn_builder.query_len = int(message)
            new_ids = self.turn_builder.turn_ids(state.get("turn_index", 0), protocol.num_video_tokens(grid, self.cfg) if grid else 0,
                                                 with_query=True)
        ids = new_ids if past_ids is None else np.concatenate([past_ids, new_ids])
        out = self.model.generate(
            input_ids=torch.from_numpy(ids).view(1, -1), frames=clip, frames_layout="TCHW",
            past_key_values=None if hf_spaces else state.get("past_key_values"), return_dict_in_generate=True, do_sample=do_sample,
            repetition_penalty=repetition_penalty, max_new_tokens=max_new_tokens,
            min_new_tokens=max_new_tokens if force_length else None, pad_token_id=self.cfg.eos_token_id, **kwargs)
        seq = out.sequences[0].cpu().numpy()
        if hf_spaces:                                                                # ref :237-238
            out.past_key_values.release()
            state["past_key_values"], state["past_ids"] = None, None
        else:
            state["past_key_values"], state["past_ids"] = out.past_key_values, seq[:-1]
        state["turn_index"] = state.get("turn_index", 0) + 1
        new_tokens = seq[len(ids):].tolist()
        self.last_generated.append(dict(span=None, prompt_ids=new_ids, tokens=new_tokens))
        return self.decode([t for t in new_tokens if t not in self.model.eos_token_ids]), state

    # --------------------------------------------------------------------------------------------------------------
    # prefill-only multiple-choice scoring
    # --------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def mcq_predict(self, clip: Optional[torch.Tensor], question: str, options: List[str], letters=("A", "B", "C", "D"),
                    frames_layout: str = "TCHW", question_prefix: str = "", question_postfix: str = "\nPlease select the correct answer.",
                    answer_prefix: str = "Answer:", abcd_previous_str: str = ": ", subtitles: Optional[str] = None):
        """ref evaluation/distributed_mcq_predictor.py:33-105: one-shot prefill of [video] + question + options + 'Answer:',
        logits of the LAST prompt position restricted to the option-letter ids (`tokenizer(': A').input_ids[-1]`, ...), argmax.
        Returns (index of the chosen option, restricted logits).  Needs tokenizer files (`self.text`)."""
        if self.text is None:
            raise ValueError("mcq_predict needs tokenizer files (pass text=TextFrontEnd(...) or a checkpoint directory)")
        letter_ids = self._mcq_letter_ids(letters, abcd_previous_str)
        grid = None
        if clip is not None:
            grid = protocol.grid_of(clip.shape[0], *_hw(clip, frames_layout), self.cfg)
        ids = self._mcq_ids(grid, question, options, question_prefix, question_postfix, answer_prefix, subtitles)
        out = self.model.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=clip, frames_layout=frames_layout,
                                  return_dict_in_generate=True, do_sample=False, repetition_penalty=1.0, max_new_tokens=1,
                                  output_logits=True, pad_token_id=self.cfg.eos_token_id)
        out.past_key_values.release()
        logits = out.logits[0].float().view(-1)[torch.as_tensor(letter_ids, device=out.logits.device)]
        return int(torch.argmax(logits)), logits.cpu()

    def _mcq_letter_ids(self, letters, abcd_previous_str):
        tok = self.text.tokenizer
        return [tok(f"{abcd_previous_str}{x}").input_ids[-1] for x in letters]                   # ref :91

    def _mcq_ids(self, grid, question, options, question_prefix, question_postfix, answer_prefix, subtitles) -> np.ndarray:
        """The full prompt ids of one multiple-choice question (ref evaluation/distributed_mcq_predictor.py:37-57)."""
        query = question_prefix + question + "\n" + "\n".join(options) + question_postfix       # ref :37
        if subtitles is not None:                                                                # ref :50-52
            query = f"This video's subtitles are listed below:\n{subtitles}\nAccording to the video and subtitles, " + query
        text = self.text.qa_text(query, continuing=False, with_video=grid is not None) + answer_prefix   # ref :56-57
        return self.text.encode(text, [grid] if grid is not None else [])

    def _model_lock(self):
        lock = getattr(self.model, "_lock", None)          # (stand-in models of the CPU tests may have no engine lock)
        return contextlib.nullcontext() if lock is None else lock

    @torch.inference_mode()
    def mcq_predict_many(self, clip: torch.Tensor, items, letters=("A", "B", "C", "D"), frames_layout: str = "TCHW",
                         question_prefix: str = "", question_postfix: str = "\nPlease select the correct answer.",
                         answer_prefix: str = "Answer:", abcd_previous_str: str = ": "):
        """Several questions about ONE clip (the shape of the reference's MCQ benchmarks: `item["questions"]` per video, ref
        evaluation/videomme/eval_your_results.py:162) for one vision tower and one long prefill instead of one per question.
        `items`: (question, options) or (question, options, subtitles) each; the keywords are `mcq_predict`'s.  Returns
        [(choice, restricted logits), ...] in item order.
        Every question's full prompt ids are built exactly as `mcq_predict` builds them; all of them share the leading ids up to and
        including <|vision_end|> (a special token: the split needs no re-tokenisation).  That prefix -- system prompt + the whole
        clip -- is prefilled ONCE, the stream is forked once per question (`StreamState.fork`, a device-side copy of the cache),
        and the question tails run as one batched prefill whose last-position logits are read.  `rope_delta` of the prefix's
        first-turn index makes the tail positions those of the one-shot prompt.  With fewer free slots than questions the tails run
        in waves of the free slots; the prefix stream and every fork are released before returning."""
        if self.text is None:
            raise ValueError("mcq_predict_many needs tokenizer files (pass text=TextFrontEnd(...) or a checkpoint directory)")
        if clip is None:
            raise ValueError("mcq_predict_many shares the prefill of a clip between questions; without a clip use mcq_predict")
        items = [tuple(it) for it in items]
        if not items:
            return []
        if any(len(it) not in (2, 3) for it in items):
            raise ValueError("each item is (question, options) or (question, options, subtitles)")
        letter_ids = self._mcq_letter_ids(letters, abcd_previous_str)
        grid = protocol.grid_of(clip.shape[0], *_hw(clip, frames_layout), self.cfg)
        all_ids = [self._mcq_ids(grid, it[0], it[1], question_prefix, question_postfix, answer_prefix, it[2] if len(it) == 3 else None)
                   for it in items]
        ends = np.flatnonzero(all_ids[0] == self.cfg.vision_end_token_id)
        if len(ends) == 0:
            raise ValueError("the prompt holds no <|vision_end|>: nothing to share between the questions")
        cut = int(ends[-1]) + 1                                                    # the shared prefix: everything up to and including it
        prefix = all_ids[0][:cut]
        for ids in all_ids:
            if len(ids) <= cut or not np.array_equal(ids[:cut], prefix):
                raise ValueError("the questions' prompts do not share their ids up to <|vision_end|>")
        model = self.model
        results: list = []
        with self._model_lock():
            if model.engine.max_slots < 2 or len(model._free_slots) < 2:
                raise RuntimeError(f"mcq_predict_many needs two free stream slots (the shared prefix + at least one fork): "
                                   f"{len(model._free_slots)} of {model.engine.max_slots} are free (raise max_streams)")
            base, forks = None, []
            try:
                out = model.generate(input_ids=torch.from_numpy(prefix).view(1, -1), frames=clip, frames_layout=frames_layout,
                                     return_dict_in_generate=True, do_sample=False, repetition_penalty=1.0, max_new_tokens=1,
                                     pad_token_id=self.cfg.eos_token_id)          # (the sampled token is discarded: it was never cached)
                base = out.past_key_values
                wave = min(len(model._free_slots), int(getattr(model, "DECODE_GROUP", 64)))
                for a in range(0, len(all_ids), wave):
                    part = all_ids[a:a + wave]
                    for _ in part:
                        forks.append(base.fork())
                    outs = model.generate_batch([dict(input_ids=torch.from_numpy(ids), state=st) for ids, st in zip(part, forks)],
                                                max_new_tokens=1, output_logits=True, repetition_penalty=1.0)
                    for o in outs:
                        lg = o.logits[0].float().view(-1)[torch.as_tensor(letter_ids, device=o.logits.device)]
                        results.append((int(torch.argmax(lg)), lg.cpu()))
                    while forks:
                        forks.pop().release()
            finally:
                for st in forks:
                    st.release()
                if base is not None:
                    base.release()
        return results

    # --------------------------------------------------------------------------------------------------------------
    # a question on the side of a running stream
    # --------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def ask(self, message, state: dict, do_sample: bool = False, repetition_penalty: float = 1.05, **kwargs):
        """A question to a stream WITHOUT touching it (ref demo/app.py lets a user talk to the model while commentary runs; there,
        and with `video_qa` on a `live_cc` state here, the question and its answer stay in the stream's cache for good).  The
        stream's cache is forked (`StreamState.fork`), the continuing text turn of `video_qa` -- `past_ids` + '<|im_end|>\n' + the
        turn -- runs on the fork, and the fork is released.  `message`, `do_sample`, `repetition_penalty`, `max_new_tokens` (512) and
        the other keyword arguments are `video_qa`'s.  Returns the response; `state` is not modified in any key (no id, no cached
        row, no repetition-penalty bit and no RNG draw of the question reaches the stream).  Recorded in `last_generated`."""
        max_new_tokens = int(kwargs.pop("max_new_tokens", 512))
        force_length = bool(kwargs.pop("force_length", False))
        with self._model_lock():       # ids, fork, turn and release as one step: no other thread advances the stream in between
            src, past_ids = state.get("past_key_values"), state.get("past_ids")
            if src is None or past_ids is None:
                raise ValueError("ask needs a stream with a cache (state['past_key_values'] and state['past_ids']); use video_qa to start one")
            if isinstance(message, str):
                if self.text is None:
                    raise ValueError("a query string needs tokenizer files (pass text=TextFrontEnd(...) or a checkpoint directory)")
                text = self.text.apply_chat_template([{"role": "user", "content": [{"type": "text", "text": message}]}], add_generation_prompt=True)
                new_ids = self.text.encode("<|im_end|>\n" + text[self.text.system_prompt_offset:], [])   # ref :218-219
            else:
                tb = self.turn_builder                       # synthetic ids: the builder's query length and draw sequence are the stream's
                keep_len, rng = tb.query_len, getattr(tb, "_rng", None)
                keep_rng = rng.get_state() if rng is not None else None
                try:
                    tb.query_len = int(message)
                    new_ids = tb.turn_ids(state.get("turn_index", 0), 0, with_query=True)      # the index video_qa uses
                finally:
                    tb.query_len = keep_len
                    if keep_rng is not None:
                        rng.set_state(keep_rng)
            ids = np.concatenate([np.asarray(past_ids), new_ids])
            fork = src.fork()
            try:
                out = self.model.generate(
                    input_ids=torch.from_numpy(ids).view(1, -1), past_key_values=fork, return_dict_in_generate=True, do_sample=do_sample,
                    repetition_penalty=repetition_penalty, max_new_tokens=max_new_tokens,
                    min_new_tokens=max_new_tokens if force_length else None, pad_token_id=self.cfg.eos_token_id, **kwargs)
                new_tokens = out.sequences[0].cpu().numpy()[len(ids):].tolist()
            finally:
                fork.release()
        self.last_generated.append(dict(span=None, prompt_ids=new_ids, tokens=new_tokens))
        return self.decode([t for t in new_tokens if t not in self.model.eos_token_ids])

    # --------------------------------------------------------------------------------------------------------------
    # offline replay of a whole clip (ref demo/infer.py:244-310)
    # --------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def live_cc_once_for_evaluation(self, query: str, video, video_start: float = 0, video_end: float = None,
                                    remote_loader: callable = None, max_new_tokens: int = 32, repetition_penalty: float = 1.05,
                                    **kwargs):
        """The reference's signature.  `video`: a registered path / `DecodedVideo` (read with `_read_video_decord_plus`'s frame
        selection for [video_start, video_end] and resized under `_spatial_resize_video`'s budget, ref :256-257), or an
        already sampled + resized uint8 clip tensor [T,3,H,W] (`frames_layout='THWC'` for decoder order).  Chunks 6,2,2,...;
        the query goes with the first turn only; do_sample is not passed, i.e. the checkpoint's generation_config decides
        (ref :297-302).  Returns [[t0, t1, text], ...].  The KV slot lives in locals like the reference's (:303-304) and is
        released before returning."""
        frames_layout = kwargs.pop("frames_layout", "TCHW")
        force_length = bool(kwargs.pop("force_length", False))
        if isinstance(video, torch.Tensor):
            clip = video
        else:
            clip, _ = V.read_video_decord_plus({"video": video, "video_start": video_start, "video_end": video_end,
                                                "remote_loader": remote_loader}, device=self.model.device)
            clip = V.spatial_resize_video(clip, device=self.model.device)
            frames_layout = "TCHW"
        state: dict = {}
        responses = []
        try:
            stop = 0.0
            for i, (a, b) in enumerate(protocol.split_clip(clip.shape[0])):
                start, stop = (0.0, self.initial_time_interval) if i == 0 else (stop, stop + self.streaming_time_interval)   # ref :270-273
                text = self._turn(clip[a:b], frames_layout, start, stop, state, query if i == 0 else None, None, None,
                                  repetition_penalty, None, None, max_new_tokens, force_length, dict(kwargs))
                responses.append([(video_start or 0) + start, (video_start or 0) + stop, text])
        finally:
            kv = state.pop("past_key_values", None)
            if kv is not None:
                kv.release()
        return responses
