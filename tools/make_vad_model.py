#!/usr/bin/env python3
"""Synthetic Silero-VAD v5 (16 kHz) model files in ggml's legacy container, and the offline definition of that format.

This restates the layout of whisper.cpp's convert-silero-vad-to-ggml.py from memory. It is UNVERIFIED against a real
converted file (none is available offline); csrc/vad_file.cpp parses exactly what this writes.

  u32  magic 0x67676d6c
  i32  len, bytes of the model-type string ("silero-16k")
  i32  x3 version (5, 0, 0)
  i32  n_encoder_layers (4); per layer i32 in-channels, out-channels, kernel size
  i32  lstm_input, lstm_hidden, final_conv_in, final_conv_out
  tensor records {i32 n_dims, i32 name_len, i32 ftype (0 f32, 1 f16), i32 ne[n_dims] in ggml order (the torch shape
  reversed), name, data}

Two seeded shapes:
  "rand": every tensor random at 1/sqrt(fan-in) scale; probabilities hover near 0.5 (numerical parity tests).
  "gate": an energy detector (segmentation and end-to-end tests): a Hann-windowed DFT basis, non-negative encoder
          weights, layer 3's bias -5 so that near-silence maps to exactly 0, input weights 0.5|N|, recurrent weights
          0.1 N, the i and o gates' bias_ih -2, a non-negative head with bias -3.
"""
import argparse
import struct

import numpy as np

GGML_MAGIC = 0x67676D6C
MODEL_TYPE = b"silero-16k"
VERSION = (5, 0, 0)
LAYERS = [(129, 128, 3), (128, 64, 3), (64, 64, 3), (64, 128, 3)]
LSTM_IN, LSTM_HID, FINAL_IN, FINAL_OUT = 128, 128, 128, 1
N_WINDOW, N_CTX_PAD, N_FFT, HOP = 512, 64, 256, 128


def tensor_specs():
    specs = [("_model.stft.forward_basis_buffer", (258, 1, 256))]
    for l, (cin, cout, k) in enumerate(LAYERS):
        specs.append((f"_model.encoder.{l}.reparam_conv.weight", (cout, cin, k)))
        specs.append((f"_model.encoder.{l}.reparam_conv.bias", (cout,)))
    specs += [("_model.decoder.rnn.weight_ih", (4 * LSTM_HID, LSTM_IN)), ("_model.decoder.rnn.weight_hh", (4 * LSTM_HID, LSTM_HID)),
              ("_model.decoder.rnn.bias_ih", (4 * LSTM_HID,)), ("_model.decoder.rnn.bias_hh", (4 * LSTM_HID,)),
              ("_model.decoder.decoder.2.weight", (1, FINAL_IN, 1)), ("_model.decoder.decoder.2.bias", (1,))]
    return specs


def fan_in(shape):
    return int(np.prod(shape[1:])) if len(shape) > 1 else 1


def make_tensors(shape: str = "rand", seed: int = 0) -> dict:
    """name -> f32 array (torch shape), in file order"""
    rng = np.random.default_rng([seed, 0 if shape == "rand" else 1])
    out = {}
    for name, shp in tensor_specs():
        n = rng.standard_normal(shp)
        if shape == "rand":
            scale = 1.0 / np.sqrt(fan_in(shp)) if len(shp) > 1 else 0.1
            if name.startswith("_model.decoder.rnn.bias"):
                scale = 1.0 / np.sqrt(LSTM_HID)
            t = n * scale
        elif shape == "gate":
            if "stft" in name:
                k = np.arange(N_FFT // 2 + 1)[:, None]
                i = np.arange(N_FFT)[None, :]
                hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
                ang = 2 * np.pi * k * i / N_FFT
                t = np.concatenate([np.cos(ang) * hann, -np.sin(ang) * hann]).reshape(shp)
            elif "encoder" in name and name.endswith("weight"):
                # layer 0 at 1/fan-in (a mean over the spectrum), the others at 1/sqrt(fan-in): a 1e-4 noise floor then
                # stays under layer 3's bias of -5 and a tone of amplitude 0.1 lies far above it
                t = np.abs(n) / (fan_in(shp) if ".0." in name else np.sqrt(fan_in(shp)))
            elif "encoder" in name:
                t = np.full(shp, -5.0 if ".3." in name else 0.0)
            elif name.endswith("weight_ih"):
                t = 0.5 * np.abs(n)
            elif name.endswith("weight_hh"):
                t = 0.1 * n
            elif name.endswith("bias_ih"):
                t = np.zeros(shp)
                t[0:LSTM_HID] = -2.0                 # i
                t[3 * LSTM_HID:4 * LSTM_HID] = -2.0  # o
            elif name.endswith("bias_hh"):
                t = np.zeros(shp)
            elif name.endswith("2.weight"):
                t = np.abs(n)
            else:
                t = np.full(shp, -3.0)
        else:
            raise ValueError(shape)
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    return out


def header_bytes(layers=LAYERS, model_type=MODEL_TYPE, magic=GGML_MAGIC, tail=(LSTM_IN, LSTM_HID, FINAL_IN, FINAL_OUT)) -> bytes:
    b = struct.pack("<I", magic) + struct.pack("<i", len(model_type)) + model_type + struct.pack("<3i", *VERSION)
    b += struct.pack("<i", len(layers))
    for l in layers:
        b += struct.pack("<3i", *l)
    return b + struct.pack("<4i", *tail)


def tensor_record(name: str, t: np.ndarray, f16: bool = False) -> bytes:
    nb = name.encode()
    b = struct.pack("<3i", t.ndim, len(nb), 1 if f16 else 0)
    b += struct.pack(f"<{t.ndim}i", *reversed(t.shape))
    return b + nb + t.astype(np.float16 if f16 else np.float32).tobytes()


def model_bytes(tensors: dict, f16_names=()) -> tuple[bytes, list[int]]:
    """the file, and the offsets at which a record (the header, then every tensor) ends"""
    b = header_bytes()
    ends = [len(b)]
    for name, t in tensors.items():
        b += tensor_record(name, t, name in f16_names)
        ends.append(len(b))
    return b, ends


def f16_default_names():
    """the tensors the f16 variant stores as f16 (the matrices; biases stay f32, as ggml converters do)"""
    return {n for n, s in tensor_specs() if len(s) > 1}


def effective_tensors(tensors: dict, f16: bool) -> dict:
    """what a loader holds after reading the file: f16 tensors rounded through f16"""
    names = f16_default_names() if f16 else set()
    return {n: (t.astype(np.float16).astype(np.float32) if n in names else t) for n, t in tensors.items()}


def write_vad_model(path: str, shape: str = "rand", seed: int = 0, f16: bool = False) -> dict:
    tensors = make_tensors(shape, seed)
    b, _ = model_bytes(tensors, f16_default_names() if f16 else ())
    with open(path, "wb") as f:
        f.write(b)
    return effective_tensors(tensors, f16)


def burst_signal(seconds: float = 6.0, seed: int = 0, bursts=((0.8, 1.6), (2.6, 3.4), (4.4, 5.2)), sr: int = 16000) -> np.ndarray:
    """tone bursts (0.3 sin 220 Hz + 0.1 sin 1300 Hz + noise) over a 1e-4 noise floor: the test signal of the VAD tests"""
    rng = np.random.default_rng([seed, 77])
    n = int(seconds * sr)
    t = np.arange(n) / sr
    x = 1e-4 * rng.standard_normal(n)
    tone = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 1300 * t) + 0.01 * rng.standard_normal(n)
    for a, b in bursts:
        x[int(a * sr):int(b * sr)] += tone[int(a * sr):int(b * sr)]
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--shape", default="gate", choices=["rand", "gate"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--f16", action="store_true")
    a = ap.parse_args()
    write_vad_model(a.out, a.shape, a.seed, a.f16)
    print(a.out)


if __name__ == "__main__":
    main()
