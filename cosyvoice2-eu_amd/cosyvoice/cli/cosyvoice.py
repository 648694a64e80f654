"""`CosyVoice2` — the API surface of cosyvoice/cli/cosyvoice.py:144-294 kept for callers (evaluation pipeline,
run_inference.py, cosyvoice2_eu): same constructor arguments, same generator methods yielding
{'tts_speech': float32 CPU tensor [1, n]}, `.sample_rate`, `add_zero_shot_spk`.  The body is new: checkpoints are read
straight from `.pt` files (no hyperpyyaml object graph; the architecture is fixed) into the HIP
engines.
"""
import logging
import os
import time

import torch

from cosyvoice.cli.frontend import CosyVoiceFrontEnd, FrontEndUnavailable, PrecomputedFrontEnd
from cosyvoice.cli.model import CosyVoice2Model


class CosyVoice2:
    flow_solver = None              # a .solver(...) view's cv2amd.solver.Solver; None: the model's flow steps and guidance rate
    join = None                     # a .joined(...) view's cv2amd.join.Join; None: the segments of a split text are yielded one by one
    stream_join = None              # a .continuous(...) view's cv2amd.join.Join; None: the segments of a split text stream as separate calls
    out_level = None                # a .level(...) view's cv2amd.level.Level; None: no level stage, the audio goes out as the vocoder gave it

    def __init__(self, model_dir, load_jit=False, load_trt=False, load_vllm=False, fp16=False, trt_concurrent=1, setting='original',
                 llm_run_id=None, flow_run_id=None, hifigan_run_id=None, final=False, backbone=None, frontend=None, state_dicts=None,
                 output_sample_rate=None, output_pcm16=False):
        """model_dir: directory with llm/flow/hift checkpoints (+ tokenizer and ONNX frontend models).
        Extra keyword-only hooks of this build: `frontend` (object with the CosyVoiceFrontEnd interface) and `state_dicts`
        (llm, flow, hift) to construct the model without files (synthetic weights, tests); `output_sample_rate` (8000, 16000, 22050,
        24000, 32000, 44100 or 48000) and `output_pcm16`: every inference_* call yields its audio at that rate and / or as int16 PCM,
        converted on the device.  `.sample_rate` then reports the output rate, `.model_sample_rate` the model's."""
        if output_sample_rate is not None:
            from cv2amd import outrate
            outrate.check_rate(output_sample_rate)                          # refused before anything is loaded
        self.output_sample_rate, self.output_pcm16 = output_sample_rate, bool(output_pcm16)
        self.sampling = None                                                # a .sampler(...) view's Sampling; None: the model's sampler and counter seed
        self.model_dir = model_dir
        self.fp16 = fp16
        self.model_sample_rate = 24000                                      # conf/cosyvoice2.yaml:8; what the frontends receive as resample_rate
        if load_jit or load_trt or load_vllm:
            logging.warning('load_jit / load_trt / load_vllm are NVIDIA-path accelerators of the reference; ignored on MI355X')
        if state_dicts is None and not os.path.exists(model_dir):
            raise ValueError('model_dir {} does not exist'.format(model_dir))
        # cosyvoice2.yaml (cli/cosyvoice.py:176-226): required next to the checkpoints, read for the run-time hyper-parameters and
        # checked against the fixed architecture; `backbone` selects qwen_pretrain_path exactly as the reference does
        from cv2amd.config import Config
        config = Config()
        if state_dicts is None:
            hyper_yaml_path = '{}/cosyvoice2.yaml'.format(model_dir)
            if not os.path.exists(hyper_yaml_path):
                raise ValueError('{} not found!'.format(hyper_yaml_path))
            overrides, qwen = {}, None
            blank = os.path.join(model_dir, 'CosyVoice-BlankEN')
            if backbone is not None:
                if backbone == 'blanken':
                    qwen = blank if os.path.exists(blank) else None
                elif backbone.startswith('hf:'):
                    qwen = backbone[3:]
                elif backbone.startswith('local:'):
                    qwen = backbone[6:]
                else:
                    qwen = backbone
            elif os.path.exists(blank) and not os.environ.get('COSYV2_IGNORE_BLANKEN'):
                qwen = blank
            if qwen:
                overrides['qwen_pretrain_path'] = qwen
                logging.info('Using LLM backbone: {}'.format(qwen))
            config = Config.from_file(hyper_yaml_path, overrides)
            self.model_sample_rate = config.sample_rate
        self.config = config
        # checkpoint selection, cli/cosyvoice.py:240-265
        if final:
            tokens = {'llm', 'flow', 'hifigan'}
        elif setting == 'original':
            tokens = set()
        else:
            tokens = set(setting.split('_'))
            invalid = tokens - {'llm', 'flow', 'hifigan'}
            if invalid:
                raise ValueError('setting should be one of "original", "llm", "flow", "hifigan", "llm_flow", "llm_hifigan", '
                                 '"flow_hifigan", "llm_flow_hifigan", but got {}'.format(setting))
        chosen = {}
        for key, run_id in (('llm', llm_run_id), ('flow', flow_run_id), ('hift', hifigan_run_id)):
            token = key if key != 'hift' else 'hifigan'
            if final or (token in tokens and run_id is not None):
                suffix = '' if final else '-{}'.format(run_id)
            else:
                suffix = '-original'
            chosen[key] = '{}/{}{}.pt'.format(model_dir, key, suffix)
        self.model = CosyVoice2Model(fp16=fp16, config=config)
        if state_dicts is not None:
            self.model.load_state_dicts(*state_dicts)
        else:
            print('Loading CosyVoice2 with\n\tLLM: {}\n\tFlow: {}\n\tHiFT: {}'.format(chosen['llm'], chosen['flow'], chosen['hift']))
            self.model.load(chosen['llm'], chosen['flow'], chosen['hift'])
        if frontend is not None:
            self.frontend = frontend
        else:
            try:
                self.frontend = CosyVoiceFrontEnd(model_dir)
            except FrontEndUnavailable as e:
                logging.warning('prompt frontend unavailable (%s); only pre-extracted prompts (add_zero_shot_spk / spk2info) will work', e)
                self.frontend = PrecomputedFrontEnd(lambda t: (_ for _ in ()).throw(FrontEndUnavailable('no tokenizer')))

    @property
    def sample_rate(self):
        """the rate of the yielded audio (callers write files with it): the output rate when one was asked for, else the model's"""
        return self.output_sample_rate if self.output_sample_rate is not None else self.model_sample_rate

    def output(self, sample_rate=None, pcm16=None):
        """A view of this object (same model, same frontend) that yields at another output rate / format: what a server uses for a
        request that asks for its own rate.  None keeps this object's setting."""
        import copy
        if sample_rate is not None:
            from cv2amd import outrate
            outrate.check_rate(sample_rate)
        view = copy.copy(self)
        view.output_sample_rate = self.output_sample_rate if sample_rate is None else sample_rate
        view.output_pcm16 = self.output_pcm16 if pcm16 is None else bool(pcm16)
        return view

    def sampler(self, seed=None, temperature=None, top_p=None, top_k=None, win_size=None, tau_r=None, greedy=None):
        """A view of this object (same model, same frontend) whose calls carry their own sampler settings and / or seed: what a server
        uses for a request that wants a reproducible, a more conservative or a livelier reading.  None keeps this object's setting (the
        model's where it has none).  seed 0 .. 2**64 - 1, temperature 0.05 .. 10, top_p (0, 1], top_k 1 .. 25, win_size 1 .. 64,
        tau_r >= 0, greedy True / False; anything else raises ValueError here, before the model is touched.  A seeded call draws the
        same uniforms and the same vocoder noise whatever else the model is serving; the segments of a split text
        use streams 0, 1, 2, ... of the one seed.  Composes with .output()."""
        import copy
        from cv2amd.sampling import Sampling
        new = Sampling(seed=seed, temperature=temperature, top_p=top_p, top_k=top_k, win_size=win_size, tau_r=tau_r, greedy=greedy).check()
        view = copy.copy(self)
        if self.sampling is not None:
            new = self.sampling.replace(**{k: getattr(new, k) for k in ('seed', 'temperature', 'top_p', 'top_k', 'win_size', 'tau_r', 'greedy')})
        view.sampling = None if new.is_default() else new
        return view

    def solver(self, steps=None, cfg_rate=None):
        """A view of this object (same model, same frontend) whose calls run the flow with their own solver settings: what a server uses
        to offer a fast and a high-quality voice from one loaded model.  steps = Euler steps 1 .. 31 (cosyvoice2.yaml: 10; measured at a 10 s utterance:
        flow call 23.6 / 14.8 / 10.4 ms at 10 / 6 / 4 steps), cfg_rate = classifier-free-guidance rate >= 0 (0.7); None keeps this object's setting (the model's where it has
        none); anything else raises ValueError here, before the model is touched.  Composes with .sampler() and .output()."""
        import copy
        from cv2amd.solver import Solver
        new = Solver(steps=steps, cfg_rate=cfg_rate).check()
        view = copy.copy(self)
        if self.flow_solver is not None:
            new = self.flow_solver.replace(steps=new.steps, cfg_rate=new.cfg_rate)
        view.flow_solver = None if new.is_default() else new
        return view

    def joined(self, pause_ms=None, trim_db=None, fade_ms=None):
        """A view of this object (same model, same frontend) whose non-streaming calls run ALL segments of a split text as one batch and
        yield ONE waveform, joined on the device: {'tts_speech': [1, n], 'segments': [(start, end), ...]} (positions in the joined 24 kHz
        signal).  pause_ms = silence between segments, 0 .. 5000 (150 when another field is set); trim_db = trim the silence at interior
        segment edges down to 20 ms around what is within trim_db of the segment's peak, 20 .. 80 (None: keep everything: the result is the
        concatenation of the plain call's segments and the pauses); fade_ms = raised-cosine fade at trimmed edges, 0 .. 20 (5 with trim_db;
        refused without it).  None keeps this object's setting; with nothing set anywhere the view is the plain object.  Anything out of
        range raises ValueError here, before the model is touched; stream=True on a joined view raises ValueError.  A generator text or a
        text of one segment takes the plain path (measured, 8 segments of 10 s: 277 ms against 955 ms one after another; same tokens as the plain calls, audio bit-equal to them only while the shared flow batch stays small, section 1).  Composes with
        .output(), .sampler() and .solver()."""
        import copy
        from cv2amd.join import Join
        new = Join(pause_ms=pause_ms, trim_db=trim_db, fade_ms=fade_ms)
        if self.join is not None:
            new = self.join.replace(pause_ms=new.pause_ms, trim_db=new.trim_db, fade_ms=new.fade_ms)
        new.check()
        view = copy.copy(self)
        view.join = None if new.is_default() else new
        if view.join is not None:
            view.stream_join = None                                         # (one view is joined or continuous: the later request holds)
        return view

    def continuous(self, pause_ms=None, trim_db=None, fade_ms=None):
        """A view of this object (same model, same frontend) whose STREAMING calls run the segments of a split text as ONE stream: one
        generator and one 24 kHz signal -- piece 0, the pause, piece 1, ... -- through ONE output record, so the resampler does not restart
        at the seams; the next segment's LLM runs ahead while the previous one's last chunks are vocoded.  Yields {'tts_speech': chunk,
        'segment': i}, the last chunk also 'segments': [(start, end), ...] (positions in the 24 kHz signal); a chunk may be empty.
        pause_ms = silence between segments, 0 .. 5000 (150 when another field is set); trim_db = gate away the silence at interior
        segment edges down to 20 ms around the loud frames, 20 .. 80 (None: keep everything); fade_ms = raised-cosine fade at gated edges,
        0 .. 5 (5 with trim_db; refused without it).  The gate is causal -- a frame is loud when within trim_db of the loudest frame SO FAR
        in the call -- and deliberately not the trim of .joined(), whose threshold needs the segment's peak and so the segment's end; the
        same text may be cut at other samples by the two.  None keeps this object's setting; with nothing set anywhere the view is the
        plain object.  Anything out of range raises ValueError here, before the model is touched; stream=False on a continuous view raises
        ValueError (use .joined() for one waveform).  A generator text or a text of one segment takes the plain streaming path.  speed
        applies per segment.  Composes with .output(), .sampler() and .solver()."""
        import copy
        from cv2amd.join import Join, check_continuous
        new = Join(pause_ms=pause_ms, trim_db=trim_db, fade_ms=fade_ms)
        if self.stream_join is not None:
            new = self.stream_join.replace(pause_ms=new.pause_ms, trim_db=new.trim_db, fade_ms=new.fade_ms)
        check_continuous(new)
        if self.out_level is not None and not new.is_default():
            self.out_level.check_stream(True)                               # (a peak target needs the call's end: not on a stream)
        view = copy.copy(self)
        view.stream_join = None if new.is_default() else new
        if view.stream_join is not None:
            view.join = None
        return view

    def level(self, gain_db=None, peak_db=None, ceiling_db=None, lookahead_ms=None, loudness_lufs=None):
        """A view of this object (same model, same frontend) whose calls set their output level on the device, just ahead of the output
        conversion: what a server uses so that two zero-shot voices come out equally loud and no call clips.  gain_db = fixed gain, -24 .. 24
        (0); ceiling_db = ceiling of the look-ahead limiter in dBFS, -12 .. 0 (-1 once any field is set): no sample leaves above it, and a
        sample with nothing over the ceiling within the look-ahead on either side is not touched at all (with gain 0 it stays bit for bit);
        lookahead_ms = 1 .. 10 (5): the limiter's gain starts to fall that long before an over and recovers that long after it; peak_db =
        scale the call so that its 24 kHz peak sits at peak_db dBFS, -24 .. 0 and <= ceiling_db -- non-streaming calls only (plain,
        coalesced, joined: the joined signal's peak); with stream=True (a continuous view included) it raises ValueError, the peak being
        known at the end only.  None keeps this object's setting; with nothing set anywhere the view is the plain object and the call takes
        exactly the path without a level stage.  Anything out of range raises ValueError here, before the model is touched.  A streaming call
        is levelled chunk by chunk to exactly the levelling of the whole call and runs lookahead_ms (5 ms by default)
        behind its vocoder: that much audio is held back until the next chunk, a non-final chunk may be empty, the last never is.  A
        continuous call has one level record over its whole signal.  Measured (profiles/level.json): the level launch over 10 s of
        audio 7 / 10 / 14 us at 1 / 5 / 10 ms look-ahead, the peak launch 21 us; nothing measurable on a 10 s non-streaming call (119.3 against 119.5 ms);
        a stream's first chunk 49.1 against 48.0 ms alone, 115.6 against 112.7 ms among 8 streams, chunk gaps unchanged.  Composes with .output(), .sampler(),
        .solver(), .joined() and .continuous().
        loudness_lufs = scale the call to that integrated loudness (ITU-R BS.1770-4: K-weighting, 400 ms blocks, the absolute and the
        relative gate; -16 for streaming services, -23 for EBU R 128), -40 .. -5, measured on the device over the call's 24 kHz signal (a joined
        call: the joined signal, pauses gated out), the gain limited to +-24 dB; gain_db stacks on top, the limiter and the ceiling run
        afterwards, so a call the limiter has to hold back ends below its target.  Non-streaming calls only, like peak_db, and not
        together with it: ValueError.  Such a call's result carries the measured loudness of its unlevelled signal as 'loudness_lufs'
        (a float, -inf for a call shorter than 400 ms or silent: its gain is then left alone).  Measured (DESIGN.md section 5,
        profiles/loudness.json): the measurement 169 us for 10 s of audio, a 10 s call 118.7 against 118.3 ms."""
        import copy
        from cv2amd.level import Level
        new = Level(gain_db=gain_db, peak_db=peak_db, ceiling_db=ceiling_db, lookahead_ms=lookahead_ms, loudness_lufs=loudness_lufs)
        if self.out_level is not None:
            new = self.out_level.replace(gain_db=new.gain_db, peak_db=new.peak_db, ceiling_db=new.ceiling_db, lookahead_ms=new.lookahead_ms,
                                         loudness_lufs=new.loudness_lufs)
        new.check()
        if self.stream_join is not None:
            new.check_stream(True)                                          # (a continuous view streams)
        view = copy.copy(self)
        view.out_level = None if new.is_default() else new
        return view

    def list_available_spks(self):
        return list(self.frontend.spk2info.keys())

    def add_zero_shot_spk(self, prompt_text, prompt_speech_16k, zero_shot_spk_id):
        assert zero_shot_spk_id != '', 'do not use empty zero_shot_spk_id'
        model_input = self.frontend.frontend_zero_shot('', prompt_text, prompt_speech_16k, self.model_sample_rate, '')
        del model_input['text']
        del model_input['text_len']
        self.frontend.spk2info[zero_shot_spk_id] = model_input
        return True

    def save_spkinfo(self):
        torch.save(self.frontend.spk2info, '{}/spk2info.pt'.format(self.model_dir))

    def _run(self, model_input, stream, speed, label, segment=0):
        start_time = time.time()
        logging.info('synthesis text {}'.format(label))
        extra = {}
        if self.output_sample_rate is not None or self.output_pcm16:
            extra = dict(output_sample_rate=self.output_sample_rate, pcm16=self.output_pcm16)
        if self.sampling is not None:                                       # (segment k of a split text: stream k under the one seed)
            extra['sampling'] = self.sampling.for_segment(segment)
        if self.flow_solver is not None:
            extra['solver'] = self.flow_solver
        if self.out_level is not None:
            extra['level'] = self.out_level
        for model_output in self.model.tts(**model_input, stream=stream, speed=speed, **extra):
            speech_len = model_output['tts_speech'].shape[1] / self.sample_rate
            logging.info('yield speech len {}, rtf {}'.format(speech_len, (time.time() - start_time) / speech_len))
            yield model_output
            start_time = time.time()

    def _segments(self, tts_text, stream, text_frontend):
        """-> (the text's segments, whether they run as ONE joined or continuous call).  A joined view refuses stream=True and a continuous
        view stream=False before any work; a generator text or a text of one segment takes the plain path."""
        if self.join is not None and stream:
            raise ValueError('a joined view yields one waveform per call: stream=True is not supported on it')
        if self.stream_join is not None and not stream:
            raise ValueError('a continuous view streams its call: stream=False is not supported on it (.joined() yields one waveform)')
        if self.out_level is not None:
            self.out_level.check_stream(stream)                             # (a peak target on a stream: refused before any work)
        texts = self.frontend.text_normalize(tts_text, split=True, text_frontend=text_frontend)
        one = self.join is not None or self.stream_join is not None
        return texts, one and len(texts) > 1 and all(isinstance(t, str) for t in texts)

    def _run_as_one(self, model_inputs, speed, label):
        """the segments as ONE call: continuous (streaming; _segments has seen stream=True) on a continuous view, else joined"""
        if self.stream_join is not None:
            return self._run_continuous(model_inputs, speed, label)
        return self._run_joined(model_inputs, speed, label)

    def _run_joined(self, model_inputs, speed, label):
        start_time = time.time()
        logging.info('synthesis text {} ({} segments, joined)'.format(label, len(model_inputs)))
        extra = {}
        if self.output_sample_rate is not None or self.output_pcm16:
            extra = dict(output_sample_rate=self.output_sample_rate, pcm16=self.output_pcm16)
        if self.sampling is not None:                                       # (segment k: stream k under the one seed, as on the plain path)
            extra['sampling'] = [self.sampling.for_segment(i) for i in range(len(model_inputs))]
        if self.flow_solver is not None:
            extra['solver'] = self.flow_solver
        if self.out_level is not None:
            extra['level'] = self.out_level
        for model_output in self.model.tts_joined(model_inputs, self.join, speed=speed, **extra):
            speech_len = model_output['tts_speech'].shape[1] / self.sample_rate
            logging.info('yield speech len {}, rtf {}'.format(speech_len, (time.time() - start_time) / speech_len))
            yield model_output

    def _run_continuous(self, model_inputs, speed, label):
        start_time = time.time()
        logging.info('synthesis text {} ({} segments, continuous)'.format(label, len(model_inputs)))
        extra = {}
        if self.output_sample_rate is not None or self.output_pcm16:
            extra = dict(output_sample_rate=self.output_sample_rate, pcm16=self.output_pcm16)
        if self.sampling is not None:                                       # (segment k: stream k under the one seed, as on the plain path)
            extra['sampling'] = [self.sampling.for_segment(i) for i in range(len(model_inputs))]
        if self.flow_solver is not None:
            extra['solver'] = self.flow_solver
        if self.out_level is not None:
            extra['level'] = self.out_level
        for model_output in self.model.tts_continuous(model_inputs, self.stream_join, speed=speed, **extra):
            speech_len = model_output['tts_speech'].shape[1] / self.sample_rate
            logging.info('yield speech len {}, rtf {}'.format(speech_len, (time.time() - start_time) / max(speech_len, 1e-9)))
            yield model_output
            start_time = time.time()

    def inference_sft(self, tts_text, spk_id, stream=False, speed=1.0, text_frontend=True):
        """cli/cosyvoice.py:81-90 (inherited by CosyVoice2): a speaker of spk2info by id, no prompt.  A CosyVoice2 model dir has no
        spk2info.pt, so an unknown `spk_id` raises the reference's KeyError (frontend.py:487)."""
        texts, joined = self._segments(tts_text, stream, text_frontend)
        if joined:
            yield from self._run_as_one([self.frontend.frontend_sft(i, spk_id) for i in texts], speed, tts_text)
            return
        for seg, i in enumerate(texts):
            model_input = self.frontend.frontend_sft(i, spk_id)
            yield from self._run(model_input, stream, speed, i, seg)

    def inference_zero_shot(self, tts_text, prompt_text, prompt_speech_16k, zero_shot_spk_id='', stream=False, speed=1.0, text_frontend=True):
        texts, joined = self._segments(tts_text, stream, text_frontend)      # (first: a joined view refuses stream=True before any work)
        prompt_text = self.frontend.text_normalize(prompt_text, split=False, text_frontend=text_frontend)
        if joined:
            for i in texts:
                if len(i) < 0.5 * len(prompt_text):
                    logging.warning('synthesis text {} too short than prompt text {}, this may lead to bad performance'.format(i, prompt_text))
            yield from self._run_as_one([self.frontend.frontend_zero_shot(i, prompt_text, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
                                         for i in texts], speed, tts_text)
            return
        for seg, i in enumerate(texts):
            if isinstance(i, str) and len(i) < 0.5 * len(prompt_text):
                logging.warning('synthesis text {} too short than prompt text {}, this may lead to bad performance'.format(i, prompt_text))
            model_input = self.frontend.frontend_zero_shot(i, prompt_text, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
            yield from self._run(model_input, stream, speed, i, seg)

    def inference_cross_lingual(self, tts_text, prompt_speech_16k, zero_shot_spk_id='', stream=False, speed=1.0, text_frontend=True):
        texts, joined = self._segments(tts_text, stream, text_frontend)
        if joined:
            yield from self._run_as_one([self.frontend.frontend_cross_lingual(i, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
                                         for i in texts], speed, tts_text)
            return
        for seg, i in enumerate(texts):
            model_input = self.frontend.frontend_cross_lingual(i, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
            yield from self._run(model_input, stream, speed, i, seg)

    def inference_vc(self, source_speech_16k, prompt_speech_16k, stream=False, speed=1.0):
        """cli/cosyvoice.py:132-139: voice conversion = the source utterance's speech tokens through flow + HiFT with the prompt's voice."""
        model_input = self.frontend.frontend_vc(source_speech_16k, prompt_speech_16k, self.model_sample_rate)
        yield from self._run(model_input, stream, speed, 'vc')

    def inference_instruct(self, *args, **kwargs):
        raise NotImplementedError('inference_instruct is not implemented for CosyVoice2!')

    def inference_instruct2(self, tts_text, instruct_text, prompt_speech_16k, zero_shot_spk_id='', stream=False, speed=1.0, text_frontend=True):
        """cli/cosyvoice.py:284-295: same three stages, the instruction rides in the prompt-text slot."""
        texts, joined = self._segments(tts_text, stream, text_frontend)
        if joined:
            yield from self._run_as_one([self.frontend.frontend_instruct2(i, instruct_text, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
                                         for i in texts], speed, tts_text)
            return
        for seg, i in enumerate(texts):
            model_input = self.frontend.frontend_instruct2(i, instruct_text, prompt_speech_16k, self.model_sample_rate, zero_shot_spk_id)
            yield from self._run(model_input, stream, speed, i, seg)
