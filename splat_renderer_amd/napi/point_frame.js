'use strict';
// node point_frame.js <positions.f32> <gradients.f32> <scales.f32> <n> <W> <H> <outPrefix>
// src/main.ts:183-190's render call in the reference's own language: PointRenderer.render with the default camera, then the
// same frame through FrameLoop.renderPoints; writes <outPrefix>rgba8 / depth / ids / loop and prints the uniform block.
// tests/test_gpu_point_renderer.py renders the same points through splat_renderer_amd.PointRenderer and compares the bytes.
const fs = require('fs');
const sr = require('./index.js');
const [posPath, gradPath, scalePath, nStr, wStr, hStr, outPrefix] = process.argv.slice(2);
const n = +nStr;
const W = +wStr;
const H = +hStr;
const f32 = (p) => {
  const b = fs.readFileSync(p);
  return new Float32Array(b.buffer, b.byteOffset, b.length / 4);
};
const device = new sr.Device(0);
const positions = device.createBufferFrom(f32(posPath));
const gradients = device.createBufferFrom(f32(gradPath));
const scales = device.createBufferFrom(f32(scalePath));
const camera = new sr.Camera();
camera.setAspect(W / H);
const uniforms = camera.uniforms(W, H);
const renderer = new sr.PointRenderer(device, null, 'rgba8unorm', n);
renderer.render(uniforms, positions, gradients, scales, W, H);
const out = (name, a) => fs.writeFileSync(outPrefix + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
out('rgba8', renderer.readPixels());
out('depth', renderer.readDepth());
out('ids', renderer.readIds());
const loop = new sr.FrameLoop(device, n, W, H);
loop.renderPoints(positions, gradients, scales, 1, 0);
out('loop', loop.readPixels());
for (const o of [renderer, loop, positions, gradients, scales]) o.destroy();
console.log(JSON.stringify({ uniforms: Array.from(uniforms) }));
