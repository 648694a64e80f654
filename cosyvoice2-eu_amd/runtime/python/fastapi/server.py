"""HTTP server of the reference (runtime/python/fastapi/server.py:40-81) over the MI355X CosyVoice2: every endpoint streams the yielded
chunks as int16 PCM, at the server's --sample_rate or the request's optional `sample_rate` form field (resampled and converted on the
device when the model was built with output_pcm16).  The optional form fields `seed`, `temperature`, `top_p`, `top_k` give a request its own
sampler settings (CosyVoice2.sampler: the same seed gives the same audio whatever else the server is doing), `flow_steps` and `cfg_rate` its own
flow solver settings (CosyVoice2.solver: Euler steps 1 .. 31, guidance rate >= 0), `pause_ms`, `trim_db` and `fade_ms` make it a joined call
(CosyVoice2.joined: the segments of a long text as one batch and one waveform, with that pause, interior silences trimmed), and with `continuous` a continuous one instead
(CosyVoice2.continuous: the segments as one stream through one resampler, the same three fields shaping its seams; the wire format is unchanged), `gain_db`, `peak_db`, `ceiling_db`, `lookahead_ms` and `loudness_lufs` its own
output level (CosyVoice2.level: a fixed gain, a peak target or a BS.1770 loudness target -- neither with `continuous`, which streams -- and a look-ahead limiter under a ceiling, on the device); values out of range answer 422.  Form / file uploads need python-multipart (as in the reference); `build_app` raises a clear error without it."""
import argparse
from typing import Optional
import os
import sys

ROOT_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT_DIR, '..'))
sys.path.insert(0, os.path.join(ROOT_DIR, '..', '..', '..'))
import wire  # noqa: E402


def generate_data(model_output):
    for i in model_output:
        yield wire.pcm_bytes(i['tts_speech'])


def request_view(cosyvoice, sample_rate=None, seed=None, temperature=None, top_p=None, top_k=None, flow_steps=None, cfg_rate=None,
                 pause_ms=None, trim_db=None, fade_ms=None, continuous=None, gain_db=None, peak_db=None, ceiling_db=None, lookahead_ms=None,
                 loudness_lufs=None):
    """the model at the request's rate (None: the server's) and with the request's sampler, flow solver, join and level settings (None: the
    model's); an unsupported rate or a setting out of range is the client's error: 422"""
    try:
        cv = cosyvoice if sample_rate is None else cosyvoice.output(sample_rate=sample_rate)
        if any(v is not None for v in (seed, temperature, top_p, top_k)):
            cv = cv.sampler(seed=seed, temperature=temperature, top_p=top_p, top_k=top_k)
        if flow_steps is not None or cfg_rate is not None:
            cv = cv.solver(steps=flow_steps, cfg_rate=cfg_rate)
        if continuous:                                                      # one stream with gated seams; with no other field: the default pause
            cv = cv.continuous(pause_ms=pause_ms if any(v is not None for v in (pause_ms, trim_db, fade_ms)) else 150, trim_db=trim_db, fade_ms=fade_ms)
        elif any(v is not None for v in (pause_ms, trim_db, fade_ms)):
            cv = cv.joined(pause_ms=pause_ms, trim_db=trim_db, fade_ms=fade_ms)
        if any(v is not None for v in (gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs)):
            cv = cv.level(gain_db=gain_db, peak_db=peak_db, ceiling_db=ceiling_db, lookahead_ms=lookahead_ms, loudness_lufs=loudness_lufs)
            if continuous:
                cv.out_level.check_stream(True)                             # (the endpoints stream a continuous request: no peak or loudness target)
        return cv
    except ValueError as e:
        from fastapi import HTTPException
        raise HTTPException(status_code=422, detail=str(e))


def build_app(cosyvoice):
    from fastapi import FastAPI, UploadFile, Form, File
    from fastapi.responses import StreamingResponse
    from fastapi.middleware.cors import CORSMiddleware
    from cosyvoice.utils.file_utils import load_wav
    app = FastAPI()
    app.add_middleware(CORSMiddleware, allow_origins=['*'], allow_credentials=True, allow_methods=['*'], allow_headers=['*'])

    def at(sample_rate, seed=None, temperature=None, top_p=None, top_k=None, flow_steps=None, cfg_rate=None, pause_ms=None, trim_db=None, fade_ms=None, continuous=None,
           gain_db=None, peak_db=None, ceiling_db=None, lookahead_ms=None, loudness_lufs=None):
        return request_view(cosyvoice, sample_rate, seed, temperature, top_p, top_k, flow_steps, cfg_rate, pause_ms, trim_db, fade_ms, continuous,
                            gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs)

    @app.get('/inference_zero_shot')
    @app.post('/inference_zero_shot')
    async def inference_zero_shot(tts_text: str = Form(), prompt_text: str = Form(), prompt_wav: UploadFile = File(), sample_rate: Optional[int] = Form(None),
                                  seed: Optional[int] = Form(None), temperature: Optional[float] = Form(None), top_p: Optional[float] = Form(None),
                                  top_k: Optional[int] = Form(None), flow_steps: Optional[int] = Form(None), cfg_rate: Optional[float] = Form(None),
                                  pause_ms: Optional[float] = Form(None), trim_db: Optional[float] = Form(None), fade_ms: Optional[float] = Form(None),
                                  continuous: Optional[bool] = Form(None), gain_db: Optional[float] = Form(None), peak_db: Optional[float] = Form(None),
                                  ceiling_db: Optional[float] = Form(None), lookahead_ms: Optional[float] = Form(None),
                                  loudness_lufs: Optional[float] = Form(None)):
        return StreamingResponse(generate_data(at(sample_rate, seed, temperature, top_p, top_k, flow_steps, cfg_rate, pause_ms, trim_db, fade_ms, continuous, gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs).inference_zero_shot(tts_text, prompt_text, load_wav(prompt_wav.file, 16000), stream=bool(continuous))))

    @app.get('/inference_cross_lingual')
    @app.post('/inference_cross_lingual')
    async def inference_cross_lingual(tts_text: str = Form(), prompt_wav: UploadFile = File(), sample_rate: Optional[int] = Form(None),
                                  seed: Optional[int] = Form(None), temperature: Optional[float] = Form(None), top_p: Optional[float] = Form(None),
                                  top_k: Optional[int] = Form(None), flow_steps: Optional[int] = Form(None), cfg_rate: Optional[float] = Form(None),
                                  pause_ms: Optional[float] = Form(None), trim_db: Optional[float] = Form(None), fade_ms: Optional[float] = Form(None),
                                  continuous: Optional[bool] = Form(None), gain_db: Optional[float] = Form(None), peak_db: Optional[float] = Form(None),
                                  ceiling_db: Optional[float] = Form(None), lookahead_ms: Optional[float] = Form(None),
                                  loudness_lufs: Optional[float] = Form(None)):
        return StreamingResponse(generate_data(at(sample_rate, seed, temperature, top_p, top_k, flow_steps, cfg_rate, pause_ms, trim_db, fade_ms, continuous, gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs).inference_cross_lingual(tts_text, load_wav(prompt_wav.file, 16000), stream=bool(continuous))))

    @app.get('/inference_instruct2')
    @app.post('/inference_instruct2')
    async def inference_instruct2(tts_text: str = Form(), instruct_text: str = Form(), prompt_wav: UploadFile = File(), sample_rate: Optional[int] = Form(None),
                                  seed: Optional[int] = Form(None), temperature: Optional[float] = Form(None), top_p: Optional[float] = Form(None),
                                  top_k: Optional[int] = Form(None), flow_steps: Optional[int] = Form(None), cfg_rate: Optional[float] = Form(None),
                                  pause_ms: Optional[float] = Form(None), trim_db: Optional[float] = Form(None), fade_ms: Optional[float] = Form(None),
                                  continuous: Optional[bool] = Form(None), gain_db: Optional[float] = Form(None), peak_db: Optional[float] = Form(None),
                                  ceiling_db: Optional[float] = Form(None), lookahead_ms: Optional[float] = Form(None),
                                  loudness_lufs: Optional[float] = Form(None)):
        return StreamingResponse(generate_data(at(sample_rate, seed, temperature, top_p, top_k, flow_steps, cfg_rate, pause_ms, trim_db, fade_ms, continuous, gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs).inference_instruct2(tts_text, instruct_text, load_wav(prompt_wav.file, 16000), stream=bool(continuous))))

    @app.get('/inference_sft')
    @app.post('/inference_sft')
    async def inference_sft(tts_text: str = Form(), spk_id: str = Form(), sample_rate: Optional[int] = Form(None),
                                  seed: Optional[int] = Form(None), temperature: Optional[float] = Form(None), top_p: Optional[float] = Form(None),
                                  top_k: Optional[int] = Form(None), flow_steps: Optional[int] = Form(None), cfg_rate: Optional[float] = Form(None),
                                  pause_ms: Optional[float] = Form(None), trim_db: Optional[float] = Form(None), fade_ms: Optional[float] = Form(None),
                                  continuous: Optional[bool] = Form(None), gain_db: Optional[float] = Form(None), peak_db: Optional[float] = Form(None),
                                  ceiling_db: Optional[float] = Form(None), lookahead_ms: Optional[float] = Form(None),
                                  loudness_lufs: Optional[float] = Form(None)):
        # CosyVoice2 has no SFT speakers of its own; a registered zero-shot speaker id plays that role (cli/cosyvoice.py:70-76)
        return StreamingResponse(generate_data(at(sample_rate, seed, temperature, top_p, top_k, flow_steps, cfg_rate, pause_ms, trim_db, fade_ms, continuous, gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs).inference_zero_shot(tts_text, '', None, zero_shot_spk_id=spk_id, stream=bool(continuous))))
    return app


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--port', type=int, default=50000)
    ap.add_argument('--model_dir', type=str, required=True)
    ap.add_argument('--sample_rate', type=int, default=None, help='rate of the PCM sent (8000, 16000, 22050, 24000, 32000, 44100, 48000); default: the model\'s 24000')
    args = ap.parse_args()
    import uvicorn
    from cosyvoice.cli.cosyvoice import CosyVoice2
    uvicorn.run(build_app(CosyVoice2(args.model_dir, final=True, output_sample_rate=args.sample_rate, output_pcm16=True)), host='0.0.0.0', port=args.port)
