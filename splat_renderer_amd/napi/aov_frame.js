'use strict';
// node aov_frame.js <props.f32> <normals.f32> <n> <W> <H> <out prefix> [pixel|quadrant]
// One whole frame through the JS Renderer with the auxiliary outputs (wantAov), and the same lists through
// ComputeShaderRenderer.render(..., wantAov); writes <prefix>{rgba8,depth,alpha,ids,staged_depth,staged_alpha,staged_ids}
// for tests/test_gpu_aov.py to compare with the Python host bit for bit.  Prints one JSON line.
const fs = require('fs');
const sr = require('./index.js');
const [propsPath, normalsPath, nStr, wStr, hStr, prefix, kernel] = process.argv.slice(2);
const n = +nStr, W = +wStr, H = +hStr;
const f32 = (p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4); };
const out = (name, a) => fs.writeFileSync(prefix + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const device = new sr.Device(0);
if (kernel) device.compositeOptions(kernel);
const props = new sr.SplatPropertyManager(device, n); props.setFromArrays(f32(propsPath));
const normals = device.createBufferFrom(f32(normalsPath));
const camera = new sr.Camera(); camera.setAspect(W / H);
const uniforms = camera.uniforms(W, H);
const r = new sr.Renderer(device, null, 'rgba8unorm', n, 16, { records: 'projected' });
r.binner.setFrameOrder('tileFirst');
r.render(uniforms, props.getPropertyBuffer(), normals, null, W, H); // (a frame without the buffers: the readers refuse)
let refused = false;
try { r.readDepth(); } catch (e) { refused = /wantAov/.test(e.message); }
for (let k = 0; k < 2; k++) r.render(uniforms, props.getPropertyBuffer(), normals, null, W, H, true); // (2nd: sync-free)
out('rgba8', r.readPixels());
out('depth', r.readDepth());
out('alpha', r.readAlpha());
out('ids', r.readIds());
// the staged composite on the frame's own records and lists
const c = new sr.ComputeShaderRenderer(device, null, 'rgba8unorm');
c.render(uniforms, props.getPropertyBuffer(), r.binner.getTileIndicesBuffer(), normals, r.projector.getProjectedBuffer(),
  r.binner.getTileCountsBuffer(), r.binner.getTileOffsetsBuffer(), 16, Math.ceil(W / 16), W, H, true);
out('staged_depth', c.readDepth());
out('staged_alpha', c.readAlpha());
out('staged_ids', c.readIds());
// the two-plane property layout (native.render_frame_planes_aov): the same frame, the same bytes
const same = (a, b) => a.length === b.length && Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength));
const rp = new sr.Renderer(device, null, 'rgba8unorm', n, 16, { records: 'projected' });
rp.binner.setFrameOrder('tileFirst');
for (let k = 0; k < 2; k++) rp.render(uniforms, props.getPropertyPlanes(), normals, null, W, H, true);
const planesEqual = same(rp.readPixels(), r.readPixels()) && same(rp.readDepth(), r.readDepth()) && same(rp.readAlpha(), r.readAlpha()) &&
  same(rp.readIds(), r.readIds());
rp.destroy();
console.log(JSON.stringify({ uniforms: Array.from(uniforms), refusedWithoutAov: refused, planesEqual, pairs: r.finish() }));
c.destroy();
r.destroy();
