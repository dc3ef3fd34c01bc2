'use strict';
// node ellipsoid_aa_frame.js <dir> <n> <W> <H>
// One anisotropic-Gaussian frame through the JS Renderer (footprint 'ellipsoid', antialiased) from
// <dir>/{pos,scl,rot,col,u}.f32 (vec4 planes, 22 uniforms); writes <dir>/out.u8 (rgba8) for tests/test_gpu_ellipsoid_aa.py to
// compare with the Python host bit for bit.  Prints one JSON line.
const fs = require('fs');
const path = require('path');
const sr = require('./index.js');
const [dir, nStr, wStr, hStr] = process.argv.slice(2);
const n = +nStr, W = +wStr, H = +hStr;
const f32 = (name) => { const b = fs.readFileSync(path.join(dir, name + '.f32')); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const device = new sr.Device(0);
const cloud = sr.GaussianCloud.fromArrays(device, { positions: f32('pos'), scales: f32('scl'), rotations: f32('rot'), colors: f32('col') });
const r = new sr.Renderer(device, null, 'rgba8unorm', n, 16, { footprint: 'ellipsoid', antialiased: true });
r.render(f32('u'), cloud, null, null, W, H);
const px = r.readPixels();
fs.writeFileSync(path.join(dir, 'out.u8'), Buffer.from(px.buffer, px.byteOffset, px.byteLength));
console.log(JSON.stringify({ n, W, H, pairs: r.finish() }));
r.destroy();
cloud.destroy();
