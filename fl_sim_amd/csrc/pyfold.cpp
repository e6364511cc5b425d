// pyfold.cpp — `fl_sim_amd._flcfold`: the C ABI of include/flcodec.h called straight from Python lists of tensors, for
// the per-round host path of every server update and every compressed message.  The entries:
//   model_fold                flc_model_fold: FedOptServer.update / avg_parameters / add_parameters / update_gradients
//                             (_fedopt.py:196-240, nodes.py:1116-1180)
//   server_fold               flc_model_fold_server: FedDyn's and pFedMe's server updates
//   avg_and_gradients         flc_avg_and_gradients: the variance-reduced servers' avg_parameters + update_gradients
//   avg_and_gradient_records  flc_avg_and_gradient_records: the same over compressed gradients
//   avg_and_gradient_sparse_records / avg_and_gradient_dense_records
//                             the same over sparse (top-k / rand-k) and dense (dithering / natural) gradient records
//   fold_records              flc_fedopt_fold_records: the server update of a round of stacked records
//   fold_dense_records        flc_fedopt_fold_dense_records: the same for dense records
//   fold_sparse_records       flc_fedopt_fold_sparse_records: the same for sparse (top-k / rand-k) records
//   fold_mixed_records        flc_fedopt_fold_mixed_records: the same for a round whose records differ in codec
//   fold_record_groups        flc_fold_record_groups: a round of records folded into several models
//   stacked_delta_record      flc_stacked_encode_delta into a wire record + flc_delta_count_nonzero_at
//   stacked_records_round     flc_stacked_encode_round into the rows of a record block
//   delta_flat                flc_delta_flatten into a new flat tensor
//   ef_accumulate             flc_ef_accumulate into a client's error memory
//   alias                     a HIP-device tensor over a pinned host tensor's memory
//
// At configs[0] (cnn_femmist_tiny: 8 tensors, 10 clients) the kernel takes ~9 us, but going through the dispatcher
// (torch.ops.flcodec.model_fold_) cost ~14 us of host time: every tensor of the 96 in the call is boxed into an IValue
// list and unboxed again.  Here each Python tensor object is unpacked in place (THPVariable_Unpack, no refcount or
// IValue traffic), checked (HIP device, dtype, contiguous, sizes) and its pointer written into the table the C ABI
// takes.  Nothing is allocated or launched before every tensor of the call has passed its checks.
//
// The entries share one layer of helpers (the anonymous namespace's first part): `Refs` owns the references an entry
// makes (fast sequences, mapping items) and releases them when the entry returns; `take` / `tensor_row` /
// `message_row` / `record_ptr` / `as_f32` check one tensor, one list of tensors, one message, one wire record, one
// weight and fill the pointer tables, reporting what they found as a `Bad` without raising, because the exception is
// the entry's own: TypeError is the Python callers' cue that nothing ran and their other path is open (move the
// messages, fold per tensor, decode densely), ValueError a mistake of theirs — and for the same finding (a list of
// the wrong length, a tensor of the wrong size) the older entries raise ValueError where the record entries raise
// TypeError.  Each entry keeps its own order of checks: which error wins when two inputs are wrong is part of its
// contract (tests/test_pyfold_contract.py, tests/test_gpu_pyfold_contract.py).  `run_on` / `on_device` make the C
// call: GIL released, the tensors' device current, a RuntimeError naming the call on a bad status; `new_flat` /
// `gradient_views` / `views_result` are the new flat gradient buffer and its per-parameter views.
//
// `alias(host_tensor, device_index)`: a HIP-device tensor over the same memory as a pinned host tensor, for the host
// server's zero-copy staging (hoststage.py): pinned host memory is mapped into every device's address space at the
// same address (checked here with hipPointerGetAttributes before the alias is made), so the fold kernels read and write
// the server's host tensors in place over PCIe.  The alias keeps the host storage alive.
#include <Python.h>
#include <torch/csrc/autograd/python_variable.h>
#include <c10/hip/HIPStream.h>
#include <ATen/ATen.h>

#include <vector>

#include "flcodec.h"

namespace {

constexpr int kMaxSrc = 16;  // messages per flc_model_fold launch

PyObject* type_error(const char* msg) {
  PyErr_SetString(PyExc_TypeError, msg);
  return nullptr;
}
PyObject* value_error(const char* msg) {
  PyErr_SetString(PyExc_ValueError, msg);
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ the helper layer
// The new references of one entry-point call, released when it returns (by any path).
struct Refs {
  std::vector<PyObject*> owned;
  Refs() { owned.reserve(8); }
  Refs(const Refs&) = delete;
  Refs& operator=(const Refs&) = delete;
  ~Refs() {
    for (PyObject* o : owned) Py_DECREF(o);
  }
  // PySequence_Fast(o): the fast sequence (read with len / items), or nullptr with TypeError(msg) set
  PyObject* fast(PyObject* o, const char* msg) {
    PyObject* f = PySequence_Fast(o, msg);
    if (f) owned.push_back(f);
    return f;
  }
  // o[key], or nullptr with the lookup's error set
  PyObject* item(PyObject* o, PyObject* key) {
    PyObject* v = PyObject_GetItem(o, key);
    if (v) owned.push_back(v);
    return v;
  }
};
inline Py_ssize_t len(PyObject* fast) { return PySequence_Fast_GET_SIZE(fast); }
inline PyObject** items(PyObject* fast) { return PySequence_Fast_ITEMS(fast); }

// a contiguous HIP tensor of `dt` on device `*dev` (-1: any HIP device, returned in *dev); nullptr if not one
const at::Tensor* usable_as(PyObject* o, at::ScalarType dt, int* dev) {
  if (!THPVariable_Check(o)) return nullptr;
  const at::Tensor& t = THPVariable_Unpack(o);
  if (!t.is_cuda() || t.scalar_type() != dt || !t.is_contiguous()) return nullptr;
  const int d = t.get_device();
  if (*dev < 0) *dev = d;
  else if (d != *dev) return nullptr;
  return &t;
}

// What a table builder found; nothing is raised except for kRaised (a Python call failed: its error is set).
enum Bad { kOk = 0, kRaised, kBadCount, kBadTensor, kBadSize };

// One fp32 tensor: its pointer into *out; its element count defines *size (`define`) or must equal it.
template <class P>
inline Bad take(PyObject* o, int* dev, int64_t* size, bool define, P* out, const at::Tensor** tensor = nullptr) {
  const at::Tensor* a = usable_as(o, at::kFloat, dev);
  if (!a) return kBadTensor;
  if (define) *size = a->numel();
  else if (a->numel() != *size) return kBadSize;
  *out = a->data_ptr<float>();
  if (tensor) *tensor = a;
  return kOk;
}

// A sequence of nt fp32 tensors into out[0..nt): the first one's finding, tensor by tensor (sizes as take's).
template <class P>
inline Bad tensor_row(PyObject** it, Py_ssize_t nt, int* dev, int64_t* sz, bool define, P* out,
                      const at::Tensor** tensors = nullptr) {
  for (Py_ssize_t t = 0; t < nt; ++t)
    if (Bad b = take(it[t], dev, sz + t, define, out + t, tensors ? tensors + t : nullptr)) return b;
  return kOk;
}

// One message's tensor list — the message itself, or message[key] — of the model's nt sizes into row[0..nt).
Bad message_row(Refs& refs, PyObject* msg, PyObject* key /* nullptr: no lookup */, const char* not_a_sequence,
                Py_ssize_t nt, int* dev, int64_t* sz, const float** row) {
  if (key && !(msg = refs.item(msg, key))) return kRaised;
  PyObject* f = refs.fast(msg, not_a_sequence);
  if (!f) return kRaised;
  if (len(f) != nt) return kBadCount;
  return tensor_row(items(f), nt, dev, sz, false, row);
}
// message_row's finding as the entry's exception: the fold entries' (a wrong count or size is the caller's mistake,
// ValueError), or the record entries' (`all_type`: every finding is the cue for the other path, TypeError)
PyObject* message_error(Bad b, bool all_type) {
  if (b == kRaised) return nullptr;
  if (b == kBadCount) return (all_type ? type_error : value_error)("every message has one tensor per model tensor");
  if (all_type) return type_error("message tensors must be contiguous fp32 HIP tensors of the model's sizes and device");
  if (b == kBadTensor) return type_error("message tensors must be contiguous fp32 HIP tensors on the model's device");
  return value_error("message tensors must match the model tensors' sizes");
}

// theta / v (either may be None: its table stays empty) of the model's nt sizes; false with the error set.  The fold
// entries raise ValueError for a wrong count or size, the record entries (`all_type`) TypeError.
bool optimizer_rows(Refs& refs, PyObject* theta, PyObject* v, Py_ssize_t nt, int* dev, int64_t* sz, bool all_type,
                    std::vector<float*>* tp, std::vector<float*>* vp) {
  for (int which = 0; which < 2; ++which) {
    PyObject* src = which == 0 ? theta : v;
    if (src == Py_None) continue;
    PyObject* f = refs.fast(src, "theta / v must be sequences of tensors");
    if (!f) return false;
    if (len(f) != nt) {
      if (all_type) type_error("theta / v need one tensor per server tensor");
      else value_error("theta / v need one tensor per model tensor");
      return false;
    }
    std::vector<float*>& out = which == 0 ? *tp : *vp;
    out.resize(nt);
    if (Bad b = tensor_row(items(f), nt, dev, sz, false, out.data())) {
      if (all_type) type_error("theta / v must match the server tensors");
      else if (b == kBadTensor) type_error("theta / v tensors must be contiguous fp32 HIP tensors on the model's device");
      else value_error("theta / v must match the model tensors' sizes");
      return false;
    }
  }
  return true;
}

// A weight as fp32 (rounded at the boundary, as torch's add_(alpha=...) does); false with the error set.
inline bool as_f32(PyObject* o, float* out) {
  const double d = PyFloat_AsDouble(o);
  if (d == -1.0 && PyErr_Occurred()) return false;
  *out = (float)d;
  return true;
}

// A wire record — a contiguous uint8 tensor on `*dev` of at least `stride` bytes, 16-B aligned: its pointer, or
// nullptr (nothing raised).
inline const void* record_ptr(PyObject* o, size_t stride, int* dev) {
  const at::Tensor* r = usable_as(o, at::kByte, dev);
  if (!r || (size_t)r->numel() < stride || reinterpret_cast<uintptr_t>(r->data_ptr()) % 16 != 0) return nullptr;
  return r->data_ptr();
}

// local / global (global nullptr: nothing subtracted) — a client's tensors and the cached model's, pair by pair of
// one size — into lp / gp / sz, their element count into *n; false with the error set (`global_not_a_sequence`,
// `bad_tensor`: the entry's TypeError texts).
bool delta_tables(Refs& refs, PyObject* loc, PyObject* glo, const char* global_not_a_sequence, const char* bad_tensor,
                  int* dev, std::vector<const float*>* lp, std::vector<const float*>* gp,
                  std::vector<int64_t>* sz, int64_t* n) {
  PyObject* fl = refs.fast(loc, "local must be a sequence of tensors");
  if (!fl) return false;
  PyObject* fg = nullptr;
  if (glo && !(fg = refs.fast(glo, global_not_a_sequence))) return false;
  const Py_ssize_t m = len(fl);
  if (m < 1 || (fg && len(fg) != m)) {
    value_error("one global tensor per local tensor, at least one");
    return false;
  }
  lp->resize(m);
  gp->resize(fg ? m : 0);
  sz->resize(m);
  *n = 0;
  for (Py_ssize_t t = 0; t < m; ++t) {
    Bad b = take(items(fl)[t], dev, &(*sz)[t], true, &(*lp)[t]);
    if (!b && fg) b = take(items(fg)[t], dev, &(*sz)[t], false, &(*gp)[t]);
    if (b) {
      if (b == kBadTensor) type_error(bad_tensor);
      else value_error("local and global tensors must have matching sizes");
      return false;
    }
    *n += (*sz)[t];
  }
  return true;
}

// The C calls of an entry: `call(stream)` — returning the flc_* status — with the GIL released and device `dev`
// current (the current device is put back after it), on the current stream of `dev`; that status.
template <class F>
inline int run_on(int dev, F&& call) {
  void* st = c10::hip::getCurrentHIPStream((c10::DeviceIndex)dev).stream();
  int rc = FLC_OK;
  Py_BEGIN_ALLOW_THREADS
  int cur = -1;
  (void)hipGetDevice(&cur);
  if (cur != dev) (void)hipSetDevice(dev);
  rc = call(st);
  if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
  Py_END_ALLOW_THREADS
  return rc;
}
// RuntimeError "<what> failed with status <rc>: <flc_last_error()>" for the C function `what`
PyObject* failed(const char* what, int rc) {
  PyErr_Format(PyExc_RuntimeError, "%s failed with status %d: %s", what, rc, flc_last_error());
  return nullptr;
}
// run_on for an entry that calls the one C function `what`: false with that RuntimeError set on a bad status
template <class F>
inline bool on_device(int dev, const char* what, F&& call) {
  const int rc = run_on(dev, call);
  if (rc != FLC_OK) failed(what, rc);
  return rc == FLC_OK;
}

// A new flat fp32 tensor of max(n, 1) elements on device `dev`; false with RuntimeError set.
bool new_flat(int64_t n, int dev, at::Tensor* flat) {
  try {
    *flat = at::empty({n > 0 ? n : 1}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, dev));
  } catch (const std::exception& e) {
    PyErr_SetString(PyExc_RuntimeError, e.what());
    return false;
  }
  return true;
}

// The gradient buffer of a model: one new flat tensor holding the parameters' sz[t] elements back to back, gv[t] its
// view shaped like parameter pt[t], gp[t] that view's pointer; false with RuntimeError set.
bool gradient_views(const std::vector<const at::Tensor*>& pt, const std::vector<int64_t>& sz, int dev, at::Tensor* flat,
                    std::vector<at::Tensor>* gv, float** gp) {
  int64_t total = 0;
  for (int64_t s : sz) total += s;
  if (!new_flat(total, dev, flat)) return false;
  gv->reserve(pt.size());
  int64_t off = 0;
  for (size_t t = 0; t < pt.size(); ++t) {
    gv->push_back(flat->narrow(0, off, sz[t]).view(pt[t]->sizes()));
    gp[t] = flat->data_ptr<float>() + off;
    off += sz[t];
  }
  return true;
}
// (list of the views, flat buffer) as the entry's result; with `set_grad` each parameter's `.grad` is set to its view
// (update_gradients' `mp.grad = ...`: same device, dtype, sizes)
PyObject* views_result(const std::vector<const at::Tensor*>& pt, const std::vector<at::Tensor>& gv,
                       const at::Tensor& flat, bool set_grad) {
  PyObject* lst = PyList_New((Py_ssize_t)gv.size());
  if (!lst) return nullptr;
  for (size_t t = 0; t < gv.size(); ++t) {
    if (set_grad) pt[t]->mutable_grad() = gv[t];
    PyObject* w = THPVariable_Wrap(gv[t]);
    if (!w) {
      Py_DECREF(lst);
      return nullptr;
    }
    PyList_SET_ITEM(lst, (Py_ssize_t)t, w);
  }
  PyObject* fl = THPVariable_Wrap(flat);
  if (!fl) {
    Py_DECREF(lst);
    return nullptr;
  }
  return Py_BuildValue("(NN)", lst, fl);
}

// ------------------------------------------------------------------------------------------------ the entry points
// model_fold(dsts, msgs, key, weights, init_mode, beta, theta, v, opt, lr, beta2, tau)
//   dsts: sequence of model tensors (accumulators); msgs: sequence of messages, each a sequence of tensors or (key
//   not None) a mapping holding one under `key`; weights: one float per message; theta / v: sequences or None.
//   More than 16 messages are folded in chained launches (init mode 2 after the first launch, the optimizer step fused
//   into the last one — the same fmaf chain as one launch).  Errors: TypeError for a tensor the fold does not take (the
//   caller then moves messages or folds per tensor), ValueError for mismatched sizes or counts.
PyObject* model_fold(PyObject*, PyObject* args) {
  PyObject *dsts, *msgs, *key, *weights, *theta, *v;
  int init_mode, opt;
  double beta, lr, beta2, tau;
  if (!PyArg_ParseTuple(args, "OOOOidOOiddd", &dsts, &msgs, &key, &weights, &init_mode, &beta, &theta, &v, &opt, &lr,
                        &beta2, &tau))
    return nullptr;
  Refs refs;
  PyObject* fd = refs.fast(dsts, "dsts must be a sequence of tensors");
  if (!fd) return nullptr;
  PyObject* fm = refs.fast(msgs, "messages must be a sequence");
  if (!fm) return nullptr;
  PyObject* fw = refs.fast(weights, "weights must be a sequence of floats");
  if (!fw) return nullptr;
  const Py_ssize_t nt = len(fd), ns = len(fm);
  if (len(fw) != ns) return value_error("one weight per message");
  if (nt == 0) Py_RETURN_NONE;
  int dev = -1;
  std::vector<float*> dp(nt), tp, vp;
  std::vector<int64_t> sz(nt);
  if (tensor_row(items(fd), nt, &dev, sz.data(), true, dp.data()))
    return type_error("model tensors must be contiguous fp32 HIP tensors on one device");
  if (!optimizer_rows(refs, theta, v, nt, &dev, sz.data(), false, &tp, &vp)) return nullptr;
  std::vector<const float*> sp((size_t)ns * nt);
  std::vector<float> w(ns);
  for (Py_ssize_t m = 0; m < ns; ++m) {
    if (!as_f32(items(fw)[m], &w[m])) return nullptr;
    if (Bad b = message_row(refs, items(fm)[m], key == Py_None ? nullptr : key, "a message is a sequence of tensors", nt,
                            &dev, sz.data(), &sp[(size_t)m * nt]))
      return message_error(b, false);
  }
  if (!on_device(dev, "flc_model_fold", [&](void* st) {
        int rc = FLC_OK;
        Py_ssize_t m0 = 0;
        do {  // chained launches of <= 16 messages: the optimizer step with the last one only
          const Py_ssize_t cnt = ns - m0 < kMaxSrc ? ns - m0 : kMaxSrc;
          const bool last = m0 + cnt >= ns;
          rc = flc_model_fold(dp.data(), sp.data() + (size_t)m0 * nt, w.data() + m0, (int)cnt, sz.data(), (int)nt,
                              m0 == 0 ? init_mode : 2, (float)beta, last && !tp.empty() ? tp.data() : nullptr,
                              last && !vp.empty() ? vp.data() : nullptr, last ? opt : FLC_OPT_AVG, lr, beta2, tau, st);
          m0 += cnt;
        } while (rc == FLC_OK && m0 < ns);
        return rc;
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// server_fold(theta, aux, msgs, key, weights, kind, fold, init_mode, inertia, c): flc_model_fold_server (FedDyn's h
// fold + average, pFedMe's average + blend: feddyn/_feddyn.py:172-184, pfedme/_pfedme.py:166-175) on Python lists, at
// most 16 messages (the caller chains longer lists).  The same checks as model_fold, the same errors.
PyObject* server_fold(PyObject*, PyObject* args) {
  PyObject *theta, *aux, *msgs, *key, *weights;
  int kind, fold, init_mode;
  double inertia, c;
  if (!PyArg_ParseTuple(args, "OOOOOiiidd", &theta, &aux, &msgs, &key, &weights, &kind, &fold, &init_mode, &inertia,
                        &c))
    return nullptr;
  Refs refs;
  PyObject* ft = refs.fast(theta, "theta must be a sequence of tensors");
  if (!ft) return nullptr;
  PyObject* fa = refs.fast(aux, "aux must be a sequence of tensors");
  if (!fa) return nullptr;
  PyObject* fm = refs.fast(msgs, "messages must be a sequence");
  if (!fm) return nullptr;
  PyObject* fw = refs.fast(weights, "weights must be a sequence of floats");
  if (!fw) return nullptr;
  const Py_ssize_t nt = len(ft), ns = len(fm);
  if (len(fw) != ns) return value_error("one weight per message");
  if (len(fa) != nt) return value_error("one aux tensor per model tensor");
  if (ns > kMaxSrc) return value_error("server_fold takes at most 16 messages");
  if (nt == 0) Py_RETURN_NONE;
  int dev = -1;
  std::vector<float*> tp(nt), ap(nt);
  std::vector<int64_t> sz(nt);
  for (Py_ssize_t t = 0; t < nt; ++t) {  // (theta and aux side by side: the first finding in that order)
    if (take(items(ft)[t], &dev, &sz[t], true, &tp[t]))
      return type_error("model tensors must be contiguous fp32 HIP tensors on one device");
    if (Bad b = take(items(fa)[t], &dev, &sz[t], false, &ap[t]))
      return b == kBadTensor ? type_error("aux tensors must be contiguous fp32 HIP tensors on the model's device")
                             : value_error("aux tensors must match the model tensors' sizes");
  }
  std::vector<const float*> sp((size_t)(ns > 0 ? ns : 1) * nt);
  std::vector<float> w(ns > 0 ? ns : 1);
  for (Py_ssize_t m = 0; m < ns; ++m) {
    if (!as_f32(items(fw)[m], &w[m])) return nullptr;
    if (Bad b = message_row(refs, items(fm)[m], key == Py_None ? nullptr : key, "a message is a sequence of tensors", nt,
                            &dev, sz.data(), &sp[(size_t)m * nt]))
      return message_error(b, false);
  }
  if (!on_device(dev, "flc_model_fold_server", [&](void* st) {
        return flc_model_fold_server(tp.data(), ap.data(), sp.data(), w.data(), (int)ns, sz.data(), (int)nt, kind, fold,
                                     init_mode, (float)inertia, c, st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// avg_and_gradients(params, grads, msgs, w_params, w_grads, inertia[, set_grad]): flc_avg_and_gradients
// (avg_parameters then update_gradients over the same messages, nodes.py:1134-1180) on Python lists: `params` folded
// in place, `grads` (one per parameter, same sizes) written from +0; every message a mapping with "parameters" and
// "gradients".  `grads` None: the gradients go into one new flat fp32 buffer on the model's device, returned as
// (list of per-parameter views, flat buffer), and with `set_grad` each parameter's `.grad` is set to its view (as
// update_gradients' `mp.grad = ...`) — the per-update Python work of the device-resident variance-reduced servers
// (views, `.grad` setters) done here.  The same checks and errors as model_fold, all before anything is allocated or
// launched; any number of messages (the C call chains them).
PyObject* avg_and_gradients(PyObject*, PyObject* args) {
  PyObject *params, *grads, *msgs, *wpar, *wgrd;
  double inertia;
  int set_grad = 0;
  if (!PyArg_ParseTuple(args, "OOOOOd|p", &params, &grads, &msgs, &wpar, &wgrd, &inertia, &set_grad)) return nullptr;
  Refs refs;
  const bool alloc = grads == Py_None;
  PyObject* seqs[5] = {params, alloc ? params : grads, msgs, wpar, wgrd};
  PyObject* f[5];
  for (int i = 0; i < 5; ++i)
    if (!(f[i] = refs.fast(seqs[i], "avg_and_gradients takes sequences"))) return nullptr;
  const Py_ssize_t nt = len(f[0]), ns = len(f[2]);
  if (len(f[1]) != nt) return value_error("one gradient buffer per parameter");
  if (len(f[3]) != ns || len(f[4]) != ns) return value_error("one weight of each kind per message");
  if (ns == 0) return value_error("avg_and_gradients needs at least one message");
  if (nt == 0) Py_RETURN_NONE;
  int dev = -1;
  std::vector<float*> pp(nt), gp(nt);
  std::vector<int64_t> sz(nt);
  std::vector<const at::Tensor*> pt(nt);
  for (Py_ssize_t t = 0; t < nt; ++t) {  // (a parameter and its buffer side by side)
    if (take(items(f[0])[t], &dev, &sz[t], true, &pp[t], &pt[t]))
      return type_error("model tensors must be contiguous fp32 HIP tensors on one device");
    if (alloc) continue;
    if (Bad b = take(items(f[1])[t], &dev, &sz[t], false, &gp[t]))
      return b == kBadTensor ? type_error("gradient buffers must be contiguous fp32 HIP tensors on the model's device")
                             : value_error("gradient buffers must match the model tensors' sizes");
  }
  std::vector<const float*> ps((size_t)ns * nt), gs((size_t)ns * nt);
  std::vector<float> wp(ns), wg(ns);
  static PyObject* const keys[2] = {PyUnicode_InternFromString("parameters"), PyUnicode_InternFromString("gradients")};
  for (Py_ssize_t m = 0; m < ns; ++m) {
    if (!as_f32(items(f[3])[m], &wp[m]) || !as_f32(items(f[4])[m], &wg[m])) return nullptr;
    for (int k = 0; k < 2; ++k)
      if (Bad b = message_row(refs, items(f[2])[m], keys[k], "a message's parameters / gradients are sequences of tensors",
                              nt, &dev, sz.data(), &(k == 0 ? ps : gs)[(size_t)m * nt]))
        return message_error(b, false);
  }
  // (every tensor checked: the gradient buffer, when asked for, is allocated now)
  at::Tensor flat;
  std::vector<at::Tensor> gv;
  if (alloc && !gradient_views(pt, sz, dev, &flat, &gv, gp.data())) return nullptr;
  if (!on_device(dev, "flc_avg_and_gradients", [&](void* st) {
        return flc_avg_and_gradients(pp.data(), gp.data(), ps.data(), gs.data(), wp.data(), wg.data(), (int)ns, sz.data(),
                                     (int)nt, (float)inertia, st);
      }))
    return nullptr;
  if (!alloc) Py_RETURN_NONE;
  return views_result(pt, gv, flat, set_grad != 0);
}

// stacked_delta_record(local, global, k, levels, seed, counter, record, count, ws): FedOptClient.communicate's delta
// (_fedopt.py:295-308) through the stacked pipeline in one C call — flc_stacked_encode_delta of cat(local - global)
// into the packed wire record `record` (a contiguous uint8 HIP tensor of at least flc_stacked_wire_layout(n, k) bytes,
// 16-B aligned; the delta is formed in the encoder's read), then, with `count` (an int64 HIP tensor), the dithering
// stage's send count (flc_delta_count_nonzero_at over the kept entries).  `ws`: the encoder's workspace (uint8).  The
// same checks as model_fold: TypeError for a tensor the encoder does not take (the caller converts and retries),
// ValueError for sizes.  An optional last argument is the top-k stage's selection order (FLC_ORDER_*, default signed).
PyObject* stacked_delta_record(PyObject*, PyObject* args) {
  PyObject *loc, *glo, *record, *count, *wso;
  long long k;
  int levels, order = FLC_ORDER_SIGNED;
  unsigned long long seed, counter;
  if (!PyArg_ParseTuple(args, "OOLiKKOOO|i", &loc, &glo, &k, &levels, &seed, &counter, &record, &count, &wso, &order))
    return nullptr;
  Refs refs;
  int dev = -1;
  std::vector<const float*> lp, gp;
  std::vector<int64_t> sz;
  int64_t n = 0;
  if (!delta_tables(refs, loc, glo, "global must be a sequence of tensors",
                    "local / global tensors must be contiguous fp32 HIP tensors on one device", &dev, &lp, &gp, &sz, &n))
    return nullptr;
  const int m = (int)sz.size();
  const at::Tensor* rec = usable_as(record, at::kByte, &dev);
  if (!rec) return type_error("the record must be a contiguous uint8 HIP tensor on the tensors' device");
  int64_t off[4] = {0, 0, 0, 0};  // norm, idx, codes, tiles
  const size_t stride = flc_stacked_wire_layout(n, k, off);
  uint8_t* rp = rec->data_ptr<uint8_t>();
  if (stride == 0 || (size_t)rec->numel() < stride || reinterpret_cast<uintptr_t>(rp) % 16 != 0)
    return value_error("the record is smaller than the wire layout or not 16-B aligned");
  int64_t* cp = nullptr;
  if (count != Py_None) {
    const at::Tensor* c = usable_as(count, at::kLong, &dev);
    if (!c || c->numel() < 1) return type_error("count must be an int64 HIP tensor on the tensors' device");
    cp = c->data_ptr<int64_t>();
  }
  const at::Tensor* ws = usable_as(wso, at::kByte, &dev);
  if (!ws) return type_error("ws must be a contiguous uint8 HIP tensor on the tensors' device");
  int32_t* idx = reinterpret_cast<int32_t*>(rp + off[1]);
  const char* what = "flc_stacked_encode_delta";  // (two calls: the one that failed is named)
  const int rc = run_on(dev, [&](void* st) {
    int r = flc_stacked_encode_delta_ord(lp.data(), gp.data(), sz.data(), m, k, order, levels, seed, counter, idx,
                                         rp + off[2], reinterpret_cast<float*>(rp + off[0]),
                                         reinterpret_cast<uint32_t*>(rp + off[3]), ws->data_ptr(), (size_t)ws->numel(),
                                         st);
    if (r == FLC_OK && cp) {
      what = "flc_delta_count_nonzero_at";
      r = flc_delta_count_nonzero_at(lp.data(), gp.data(), sz.data(), m, idx, k, cp, st);
    }
    return r;
  });
  if (rc != FLC_OK) return failed(what, rc);
  Py_RETURN_NONE;
}

// delta_flat(local, global): a new flat fp32 tensor = cat(local_t - global_t) (flc_delta_flatten) on the tensors'
// device — the deferred compressed message's snapshot of its delta (compressed.py).  TypeError (nothing allocated)
// for a tensor that is not a contiguous fp32 HIP tensor of one device.
PyObject* delta_flat(PyObject*, PyObject* args) {
  PyObject *loc, *glo;
  if (!PyArg_ParseTuple(args, "OO", &loc, &glo)) return nullptr;
  Refs refs;
  int dev = -1;
  std::vector<const float*> lp, gp;
  std::vector<int64_t> sz;
  int64_t n = 0;
  if (!delta_tables(refs, loc, glo, "global must be a sequence of tensors",
                    "local / global tensors must be contiguous fp32 HIP tensors on one device", &dev, &lp, &gp, &sz, &n))
    return nullptr;
  at::Tensor out;
  if (!new_flat(n, dev, &out)) return nullptr;
  if (n == 0) out = out.narrow(0, 0, 0);
  float* op = out.data_ptr<float>();
  if (!on_device(dev, "flc_delta_flatten", [&](void* st) {
        return flc_delta_flatten(lp.data(), gp.data(), sz.data(), (int)sz.size(), op, st);
      }))
    return nullptr;
  return THPVariable_Wrap(out);
}

// ef_accumulate(local, global_or_None, e): e += cat(local_t - global_t) in place (flc_ef_accumulate; None: e +=
// cat(local_t)) — an error-feedback message's accumulate into the client's memory (feedback.py), `e` a contiguous fp32
// HIP tensor holding the tensors' element count.  TypeError (nothing launched) for a tensor that is not a contiguous
// fp32 HIP tensor of e's device; ValueError for mismatched sizes.
PyObject* ef_accumulate(PyObject*, PyObject* args) {
  PyObject *loc, *glo, *mem;
  if (!PyArg_ParseTuple(args, "OOO", &loc, &glo, &mem)) return nullptr;
  Refs refs;
  int dev = -1;
  const at::Tensor* et = usable_as(mem, at::kFloat, &dev);
  if (!et) return type_error("the memory must be a contiguous fp32 HIP tensor");
  const bool sub = glo != Py_None;
  std::vector<const float*> lp, gp;
  std::vector<int64_t> sz;
  int64_t n = 0;
  if (!delta_tables(refs, loc, sub ? glo : nullptr, "global must be a sequence of tensors or None",
                    "local / global tensors must be contiguous fp32 HIP tensors on the memory's device", &dev, &lp, &gp,
                    &sz, &n))
    return nullptr;
  if (et->numel() != n) return value_error("the memory must hold the tensors' element count");
  float* ep = et->data_ptr<float>();
  if (!on_device(dev, "flc_ef_accumulate", [&](void* st) {
        return flc_ef_accumulate(lp.data(), sub ? gp.data() : nullptr, sz.data(), (int)sz.size(), ep, st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// stacked_records_round(flats, seeds, counters, k, levels, records, counts, ws): the deferred messages of a round in
// one C call and one encode launch chain — flc_stacked_encode_round of the flat deltas, one Philox (seed, counter) per
// message, into the rows of the [C, >= stride] record block (row c equals client c's one-message record); its select
// writes the send counts counts[c] itself (no count launches).  An optional last argument is the round's selection
// order (FLC_ORDER_*, default signed).
PyObject* stacked_records_round(PyObject*, PyObject* args) {
  PyObject *flats, *seeds, *recs, *counts, *wso, *ctrs;
  long long k;
  int levels, order = FLC_ORDER_SIGNED;
  if (!PyArg_ParseTuple(args, "OOOLiOOO|i", &flats, &seeds, &ctrs, &k, &levels, &recs, &counts, &wso, &order))
    return nullptr;
  Refs refs;
  PyObject* seqs[3] = {flats, seeds, counts};
  PyObject* f[3];
  for (int i = 0; i < 3; ++i)
    if (!(f[i] = refs.fast(seqs[i], "stacked_records_round takes sequences"))) return nullptr;
  const Py_ssize_t C = len(f[0]);
  if (C < 1 || len(f[1]) != C || len(f[2]) != C)
    return value_error("one seed and one count per client, at least one client");
  PyObject* fc = refs.fast(ctrs, "stacked_records_round takes a sequence of counters");
  if (!fc) return nullptr;
  if (len(fc) != C) return value_error("one counter per client");
  std::vector<uint64_t> ct64(C);
  for (Py_ssize_t c = 0; c < C; ++c) {
    ct64[c] = (uint64_t)PyLong_AsUnsignedLongLongMask(items(fc)[c]);
    if (PyErr_Occurred()) return nullptr;
  }
  int dev = -1;
  int64_t n = -1;
  std::vector<const float*> xp(C);
  std::vector<uint64_t> sd(C);
  std::vector<int64_t*> cp(C);
  for (Py_ssize_t c = 0; c < C; ++c) {
    if (Bad b = take(items(f[0])[c], &dev, &n, c == 0, &xp[c]))
      return b == kBadTensor ? type_error("flat deltas must be contiguous fp32 HIP tensors on one device")
                             : value_error("flat deltas must all have one size");
    sd[c] = (uint64_t)PyLong_AsUnsignedLongLongMask(items(f[1])[c]);
    if (PyErr_Occurred()) return nullptr;
    const at::Tensor* ct = usable_as(items(f[2])[c], at::kLong, &dev);
    if (!ct || ct->numel() < 1) return type_error("counts must be int64 HIP tensors on the deltas' device");
    cp[c] = ct->data_ptr<int64_t>();
  }
  int64_t off[4] = {0, 0, 0, 0};  // norm, idx, codes, tiles
  const size_t stride = flc_stacked_wire_layout(n, k, off);
  if (stride == 0) return value_error("bad wire shape");
  if (!THPVariable_Check(recs)) return type_error("records must be a uint8 HIP tensor");
  const at::Tensor& rb = THPVariable_Unpack(recs);
  if (!rb.is_cuda() || rb.get_device() != dev || rb.scalar_type() != at::kByte || rb.dim() != 2 || !rb.is_contiguous() ||
      rb.size(0) != C || rb.size(1) < (int64_t)stride || rb.size(1) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(rb.data_ptr()) % 16 != 0)
    return value_error("records must be a contiguous [clients, >= stride] uint8 block (16-B rows) on the device");
  const at::Tensor* ws = usable_as(wso, at::kByte, &dev);
  if (!ws) return type_error("ws must be a contiguous uint8 HIP tensor on the deltas' device");
  uint8_t* base = rb.data_ptr<uint8_t>();
  const int64_t rs = rb.size(1);
  std::vector<int32_t*> ip(C);
  std::vector<uint8_t*> kp(C);
  std::vector<float*> np(C);
  std::vector<uint32_t*> tp(C);
  for (Py_ssize_t c = 0; c < C; ++c) {
    uint8_t* r = base + c * rs;
    np[c] = reinterpret_cast<float*>(r + off[0]);
    ip[c] = reinterpret_cast<int32_t*>(r + off[1]);
    kp[c] = r + off[2];
    tp[c] = reinterpret_cast<uint32_t*>(r + off[3]);
  }
  if (!on_device(dev, "flc_stacked_encode_round", [&](void* st) {
        return flc_stacked_encode_round_ord(xp.data(), (int)C, n, k, order, levels, sd.data(), ct64.data(), ip.data(),
                                            kp.data(), np.data(), tp.data(), cp.data(), ws->data_ptr(),
                                            (size_t)ws->numel(), st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// What a uniform round's records are — flc_record_kind with (k, levels), (k) or (format, levels, bits) — and what the
// record entries need of it: the layout's size, the C entry of each server form and that entry's name.
enum ServerForm { kFedOptForm = 0, kGradientForm = 1, kGroupForm = 2 };
struct RecordShape {
  int kind;  // FLC_REC_STACKED, FLC_REC_SPARSE or FLC_REC_DENSE
  long long k;
  int format, levels, bits;

  // bytes of one record of n elements; 0 for a shape no layout takes (an unknown kind included)
  size_t stride(long long n) const {
    int64_t off[4];
    switch (kind) {
      case FLC_REC_STACKED: return flc_stacked_wire_layout(n, k, off);
      case FLC_REC_SPARSE: return flc_sparse_wire_layout(n, k, off);
      case FLC_REC_DENSE: return flc_dense_wire_layout(n, format, bits, off);
      default: return 0;
    }
  }
  const char* name(ServerForm form) const {
    static const char* const kNames[3][3] = {
        {"flc_fedopt_fold_records", "flc_avg_and_gradient_records", "flc_fold_record_groups"},
        {"flc_fedopt_fold_sparse_records", "flc_avg_and_gradient_sparse_records", "flc_fold_sparse_record_groups"},
        {"flc_fedopt_fold_dense_records", "flc_avg_and_gradient_dense_records", "flc_fold_dense_record_groups"}};
    return kNames[kind][form];
  }
  int fedopt(const void* const* recs, const float* w, int nr, long long n, float* const* delta, float* const* theta,
             float* const* v, const int64_t* sz, int nt, float beta0, int opt, double lr, double beta2, double tau,
             void* st) const {
    if (kind == FLC_REC_SPARSE)
      return flc_fedopt_fold_sparse_records(recs, w, nr, n, k, delta, theta, v, sz, nt, beta0, opt, lr, beta2, tau, st);
    if (kind == FLC_REC_DENSE)
      return flc_fedopt_fold_dense_records(recs, w, nr, n, format, levels, bits, delta, theta, v, sz, nt, beta0, opt,
                                           lr, beta2, tau, st);
    return flc_fedopt_fold_records(recs, w, nr, n, k, levels, delta, theta, v, sz, nt, beta0, opt, lr, beta2, tau, st);
  }
  int gradient(float* const* params, float* const* grads, const float* const* srcs, const void* const* recs,
               const float* wp, const float* wg, int ns, long long n, const int64_t* sz, int nt, float inertia,
               void* st) const {
    if (kind == FLC_REC_SPARSE)
      return flc_avg_and_gradient_sparse_records(params, grads, srcs, recs, wp, wg, ns, n, k, sz, nt, inertia, st);
    if (kind == FLC_REC_DENSE)
      return flc_avg_and_gradient_dense_records(params, grads, srcs, recs, wp, wg, ns, n, format, levels, bits, sz, nt,
                                                inertia, st);
    return flc_avg_and_gradient_records(params, grads, srcs, recs, wp, wg, ns, n, k, levels, sz, nt, inertia, st);
  }
  int groups(const void* const* recs, const float* w, const int32_t* group_of, int nr, long long n, float* const* dsts,
             int ng, const int64_t* sz, int nt, void* st) const {
    if (kind == FLC_REC_SPARSE) return flc_fold_sparse_record_groups(recs, w, group_of, nr, n, k, dsts, ng, sz, nt, st);
    if (kind == FLC_REC_DENSE)
      return flc_fold_dense_record_groups(recs, w, group_of, nr, n, format, levels, bits, dsts, ng, sz, nt, st);
    return flc_fold_record_groups(recs, w, group_of, nr, n, k, levels, dsts, ng, sz, nt, st);
  }
};
inline RecordShape stacked_shape(long long k, int levels) { return {FLC_REC_STACKED, k, 0, levels, 0}; }
inline RecordShape sparse_shape(long long k) { return {FLC_REC_SPARSE, k, 0, 0, 0}; }
inline RecordShape dense_shape(int format, int levels, int bits) { return {FLC_REC_DENSE, 0, format, levels, bits}; }

// The FedOpt record entries' front half: the record, weight and server-tensor sequences, one weight per record, the
// server tensors (δ, then θ / v) of one device holding n elements.  `rows()` — the entry's own per-record tables —
// runs after the counts and before any tensor is looked at; false from it, or from here, with the error set.
struct ServerTables {
  PyObject *recs = nullptr, *weights = nullptr;  // fast sequences of nr items
  Py_ssize_t nr = 0, nt = 0;
  int dev = -1;
  std::vector<float*> dp, tp, vp;
  std::vector<int64_t> sz;
  float* const* theta() const { return tp.empty() ? nullptr : tp.data(); }
  float* const* v() const { return vp.empty() ? nullptr : vp.data(); }
};
template <class F>
bool server_tables(Refs& refs, const char* not_sequences, const char* nothing_to_fold, PyObject* recs,
                   PyObject* weights, PyObject* delta, PyObject* theta, PyObject* v, long long n, F&& rows,
                   ServerTables* s) {
  PyObject* fd = nullptr;
  if (!(s->recs = refs.fast(recs, not_sequences)) || !(s->weights = refs.fast(weights, not_sequences)) ||
      !(fd = refs.fast(delta, not_sequences)))
    return false;
  s->nr = len(s->recs), s->nt = len(fd);
  if (len(s->weights) != s->nr) return value_error("one weight per record"), false;
  if (s->nr < 1 || s->nt < 1) return type_error(nothing_to_fold), false;
  if (!rows()) return false;
  s->dp.resize(s->nt);
  s->sz.resize(s->nt);
  if (tensor_row(items(fd), s->nt, &s->dev, s->sz.data(), true, s->dp.data()))
    return type_error("server tensors must be contiguous fp32 HIP tensors on one device"), false;
  int64_t total = 0;
  for (int64_t x : s->sz) total += x;
  if (total != n) return type_error("the server tensors do not hold the records' element count"), false;
  return optimizer_rows(refs, theta, v, s->nt, &s->dev, s->sz.data(), true, &s->tp, &s->vp);
}

// fold_records(records, weights, n, k, levels, delta, theta, v, beta0, opt, lr, beta2, tau): the server update of a
// round of stacked records (flc_fedopt_fold_records) on Python lists.  TypeError (nothing launched) when a tensor is
// not what the pass takes — the server tensors contiguous fp32 HIP tensors of one device summing to n, the records
// 16-B aligned uint8 tensors of at least the wire layout's bytes on that device — so the caller can take its other
// path; theta / v None: the fold alone / no second moment.
// (fold_records_of: one worker for the three uniform kinds, by the records' RecordShape)
PyObject* fold_records_of(const RecordShape& shape, PyObject* recs, PyObject* weights, long long n, PyObject* delta,
                          PyObject* theta, PyObject* v, double beta0, int opt, double lr, double beta2, double tau) {
  Refs refs;
  ServerTables s;
  if (!server_tables(refs, "fold_records takes sequences", "fold_records needs records and server tensors", recs,
                     weights, delta, theta, v, n, [] { return true; }, &s))
    return nullptr;
  const size_t stride = shape.stride(n);
  if (stride == 0) return value_error("bad wire shape");
  std::vector<const void*> rp(s.nr);
  std::vector<float> w(s.nr);
  for (Py_ssize_t c = 0; c < s.nr; ++c) {
    if (!(rp[c] = record_ptr(items(s.recs)[c], stride, &s.dev)))
      return type_error("records must be 16-B aligned uint8 HIP tensors of the wire layout on the server's device");
    if (!as_f32(items(s.weights)[c], &w[c])) return nullptr;
  }
  if (!on_device(s.dev, shape.name(kFedOptForm), [&](void* st) {
        return shape.fedopt(rp.data(), w.data(), (int)s.nr, n, s.dp.data(), s.theta(), s.v(), s.sz.data(), (int)s.nt,
                            (float)beta0, opt, lr, beta2, tau, st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}
PyObject* fold_records(PyObject*, PyObject* args) {
  PyObject *recs, *weights, *delta, *theta, *v;
  long long n, k;
  int levels, opt;
  double beta0, lr, beta2, tau;
  if (!PyArg_ParseTuple(args, "OOLLiOOOdiddd", &recs, &weights, &n, &k, &levels, &delta, &theta, &v, &beta0, &opt, &lr,
                        &beta2, &tau))
    return nullptr;
  return fold_records_of(stacked_shape(k, levels), recs, weights, n, delta, theta, v, beta0, opt, lr, beta2, tau);
}
// fold_sparse_records(records, weights, n, k, delta, theta, v, beta0, opt, lr, beta2, tau): the same for a round of
// sparse records (flc_fedopt_fold_sparse_records; the flc_sparse_wire_layout(n, k) layout of a top-k / rand-k message)
PyObject* fold_sparse_records(PyObject*, PyObject* args) {
  PyObject *recs, *weights, *delta, *theta, *v;
  long long n, k;
  int opt;
  double beta0, lr, beta2, tau;
  if (!PyArg_ParseTuple(args, "OOLLOOOdiddd", &recs, &weights, &n, &k, &delta, &theta, &v, &beta0, &opt, &lr, &beta2,
                        &tau))
    return nullptr;
  return fold_records_of(sparse_shape(k), recs, weights, n, delta, theta, v, beta0, opt, lr, beta2, tau);
}
// fold_dense_records(records, weights, n, format, levels, bits, delta, theta, v, beta0, opt, lr, beta2, tau): the same
// for a round of dense records (flc_fedopt_fold_dense_records; the flc_dense_wire_layout(n, format, bits) layout)
PyObject* fold_dense_records(PyObject*, PyObject* args) {
  PyObject *recs, *weights, *delta, *theta, *v;
  long long n;
  int format, levels, bits, opt;
  double beta0, lr, beta2, tau;
  if (!PyArg_ParseTuple(args, "OOLiiiOOOdiddd", &recs, &weights, &n, &format, &levels, &bits, &delta, &theta, &v, &beta0,
                        &opt, &lr, &beta2, &tau))
    return nullptr;
  if (format < 0) return value_error("bad wire shape");  // (before anything else is looked at)
  return fold_records_of(dense_shape(format, levels, bits), recs, weights, n, delta, theta, v, beta0, opt, lr, beta2,
                         tau);
}

// A sequence of `want` Python ints into *out; false with the error set (TypeError for another length).
template <class T>
bool int_row(Refs& refs, PyObject* o, Py_ssize_t want, std::vector<T>* out) {
  PyObject* f = refs.fast(o, "fold_mixed_records takes sequences");
  if (!f) return false;
  if (len(f) != want) {
    type_error("one kind, k, format, levels and bits per record");
    return false;
  }
  out->resize(want);
  for (Py_ssize_t c = 0; c < want; ++c) {
    const long long x = PyLong_AsLongLong(items(f)[c]);
    if (x == -1 && PyErr_Occurred()) return false;
    (*out)[c] = (T)x;
  }
  return true;
}

// fold_mixed_records(records, weights, n, kinds, ks, formats, levels, bits, delta, theta, v, beta0, opt, lr, beta2,
// tau): the server update of a round whose records differ in codec (flc_fedopt_fold_mixed_records) on Python lists —
// one descriptor (flc_record_kind, k, format, levels, bits) per record; a FLC_REC_FLAT record is the message's decoded
// fp32 vector of n elements.  TypeError (nothing launched) when a tensor is not what the pass takes, as fold_records
// raises it: the server tensors contiguous fp32 HIP tensors of one device summing to n, every record a 16-B aligned
// tensor on that device holding its own layout's bytes (uint8) or the n elements (fp32).
PyObject* fold_mixed_records(PyObject*, PyObject* args) {
  PyObject *recs, *weights, *kinds, *ks, *fmts, *lvs, *bts, *delta, *theta, *v;
  long long n;
  int opt;
  double beta0, lr, beta2, tau;
  if (!PyArg_ParseTuple(args, "OOLOOOOOOOOdiddd", &recs, &weights, &n, &kinds, &ks, &fmts, &lvs, &bts, &delta, &theta, &v,
                        &beta0, &opt, &lr, &beta2, &tau))
    return nullptr;
  Refs refs;
  ServerTables s;
  std::vector<int32_t> kd, fm, lv, bt;
  std::vector<int64_t> kk;
  auto descriptors = [&] {
    return int_row(refs, kinds, s.nr, &kd) && int_row(refs, ks, s.nr, &kk) && int_row(refs, fmts, s.nr, &fm) &&
           int_row(refs, lvs, s.nr, &lv) && int_row(refs, bts, s.nr, &bt);
  };
  if (!server_tables(refs, "fold_mixed_records takes sequences", "fold_mixed_records needs records and server tensors",
                     recs, weights, delta, theta, v, n, descriptors, &s))
    return nullptr;
  const Py_ssize_t nr = s.nr;
  std::vector<const void*> rp(nr);
  std::vector<float> w(nr);
  for (Py_ssize_t c = 0; c < nr; ++c) {
    if (kd[c] == FLC_REC_FLAT) {
      int64_t want = n;
      const float* x = nullptr;
      if (take(items(s.recs)[c], &s.dev, &want, false, &x) || reinterpret_cast<uintptr_t>(x) % 16 != 0)
        return type_error("a flat record must be a 16-B aligned contiguous fp32 HIP tensor of n elements on the server's device");
      rp[c] = x;
    } else {
      const size_t stride = RecordShape{kd[c], kk[c], fm[c], lv[c], bt[c]}.stride(n);
      if (stride == 0) return value_error("bad wire shape");
      if (!(rp[c] = record_ptr(items(s.recs)[c], stride, &s.dev)))
        return type_error("records must be 16-B aligned uint8 HIP tensors of the wire layout on the server's device");
    }
    if (!as_f32(items(s.weights)[c], &w[c])) return nullptr;
  }
  if (!on_device(s.dev, "flc_fedopt_fold_mixed_records", [&](void* st) {
        return flc_fedopt_fold_mixed_records(rp.data(), w.data(), (int)nr, n, kd.data(), kk.data(), fm.data(), lv.data(),
                                             bt.data(), s.dp.data(), s.theta(), s.v(), s.sz.data(), (int)s.nt,
                                             (float)beta0, opt, lr, beta2, tau, st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// fold_record_groups(records, weights, dsts, n, k, levels): a round whose stacked records fall into groups, each
// folded in place into its own model (flc_fold_record_groups) on Python lists — records / weights / dsts hold one
// sequence per group (SCAFFOLD: θ and c; IFCA: the clusters with messages).  TypeError (nothing launched) when a tensor
// is not what the pass takes — every group's tensors contiguous fp32 HIP tensors of one device holding, tensor by
// tensor, the first group's element counts summing to n, no tensor in two groups, the records 16-B aligned uint8
// tensors of at least the wire layout's bytes on that device — so the caller can take its other path.
PyObject* fold_record_groups(PyObject*, PyObject* args) {
  PyObject *recs, *weights, *dsts;
  long long n, k;
  int levels;
  if (!PyArg_ParseTuple(args, "OOOLLi", &recs, &weights, &dsts, &n, &k, &levels)) return nullptr;
  Refs refs;
  const char* const not_seq = "fold_record_groups takes sequences of sequences";
  PyObject *fr = refs.fast(recs, not_seq), *fw = fr ? refs.fast(weights, not_seq) : nullptr,
           *fd = fw ? refs.fast(dsts, not_seq) : nullptr;
  if (!fd) return nullptr;
  const Py_ssize_t ng = len(fd);
  if (ng < 1 || len(fr) != ng || len(fw) != ng)
    return type_error("fold_record_groups needs one record list, weight list and tensor list per group");
  const RecordShape shape = stacked_shape(k, levels);  // (the grouped fold's only one-call entry)
  const size_t stride = shape.stride(n);
  if (stride == 0) return value_error("bad wire shape");
  int dev = -1;
  std::vector<float*> dp;
  std::vector<int64_t> sz;
  std::vector<const void*> rp;
  std::vector<float> w;
  std::vector<int32_t> gof;
  for (Py_ssize_t g = 0; g < ng; ++g) {
    PyObject* ft = refs.fast(items(fd)[g], not_seq);
    if (!ft) return nullptr;
    const Py_ssize_t nt = len(ft);
    if (nt < 1 || (g > 0 && (size_t)nt != sz.size()))
      return type_error("every group needs the first group's number of tensors");
    if (g == 0) sz.resize(nt);
    int64_t total = 0;
    for (Py_ssize_t t = 0; t < nt; ++t) {
      float* q = nullptr;
      if (Bad b = take(items(ft)[t], &dev, &sz[t], g == 0, &q))
        return type_error(b == kBadTensor ? "server tensors must be contiguous fp32 HIP tensors on one device"
                                          : "every group's tensors must match the first group's sizes");
      total += sz[t];
      if (sz[t] > 0)
        for (float* other : dp)
          if (other == q) return type_error("a server tensor in two places");
      dp.push_back(q);
    }
    if (total != n) return type_error("the server tensors do not hold the records' element count");
    PyObject* frg = refs.fast(items(fr)[g], not_seq);
    PyObject* fwg = frg ? refs.fast(items(fw)[g], not_seq) : nullptr;
    if (!fwg) return nullptr;
    const Py_ssize_t nr = len(frg);
    if (len(fwg) != nr) return value_error("one weight per record");
    for (Py_ssize_t c = 0; c < nr; ++c) {
      const void* r = record_ptr(items(frg)[c], stride, &dev);
      if (!r) return type_error("records must be 16-B aligned uint8 HIP tensors of the wire layout on the server's device");
      rp.push_back(r);
      float wc;
      if (!as_f32(items(fwg)[c], &wc)) return nullptr;
      w.push_back(wc);
      gof.push_back((int32_t)g);
    }
  }
  if (!on_device(dev, shape.name(kGroupForm), [&](void* st) {
        return shape.groups(rp.data(), w.data(), gof.data(), (int)rp.size(), n, dp.data(), (int)ng, sz.data(),
                            (int)sz.size(), st);
      }))
    return nullptr;
  Py_RETURN_NONE;
}

// avg_and_gradient_records(params, msgs, records, w_params, w_grads, n, k, levels, inertia, set_grad): a
// variance-reduced round whose gradients are stacked records (flc_avg_and_gradient_records) on Python lists.  `params`
// folded in place from every message's "parameters" (`msgs` None: left untouched — update_gradients alone, `w_params`
// unused); the gradients decoded and folded into one new flat fp32 buffer on the model's device, returned as (list of
// per-parameter views, flat buffer); with `set_grad` each parameter's `.grad` is set to its view.  TypeError (nothing
// allocated or launched) when a tensor is not what the pass takes, as fold_records and avg_and_gradients raise it.
// (avg_and_gradient_records_of: one worker for the three uniform kinds, as fold_records_of is the FedOpt entries')
PyObject* avg_and_gradient_records_of(const RecordShape& shape, PyObject* params, PyObject* msgs, PyObject* recs,
                                      PyObject* wpar, PyObject* wgrd, long long n, double inertia, int set_grad) {
  Refs refs;
  const bool p_on = msgs != Py_None;
  PyObject* seqs[5] = {params, recs, wgrd, p_on ? msgs : recs, p_on ? wpar : wgrd};
  PyObject* f[5];
  for (int i = 0; i < 5; ++i)
    if (!(f[i] = refs.fast(seqs[i], "avg_and_gradient_records takes sequences"))) return nullptr;
  const Py_ssize_t nt = len(f[0]), ns = len(f[1]);
  if (len(f[2]) != ns || len(f[3]) != ns || len(f[4]) != ns)
    return value_error("one record, one message and one weight of each kind per message");
  if (ns < 1 || nt < 1) return type_error("avg_and_gradient_records needs records and model tensors");
  int dev = -1;
  std::vector<float*> pp(nt), gp(nt);
  std::vector<int64_t> sz(nt);
  std::vector<const at::Tensor*> pt(nt);
  if (tensor_row(items(f[0]), nt, &dev, sz.data(), true, pp.data(), pt.data()))
    return type_error("model tensors must be contiguous fp32 HIP tensors on one device");
  int64_t total = 0;
  for (int64_t s : sz) total += s;
  if (total != n) return type_error("the model tensors do not hold the records' element count");
  const size_t stride = shape.stride(n);
  if (stride == 0) return value_error("bad wire shape");
  std::vector<const void*> rp(ns);
  std::vector<const float*> ps(p_on ? (size_t)ns * nt : 0);
  std::vector<float> wp(ns), wg(ns);
  static PyObject* const key = PyUnicode_InternFromString("parameters");
  for (Py_ssize_t m = 0; m < ns; ++m) {
    if (!(rp[m] = record_ptr(items(f[1])[m], stride, &dev)))
      return type_error("records must be 16-B aligned uint8 HIP tensors of the wire layout on the model's device");
    if (!as_f32(items(f[2])[m], &wg[m])) return nullptr;
    if (!p_on) continue;
    if (!as_f32(items(f[4])[m], &wp[m])) return nullptr;
    if (Bad b = message_row(refs, items(f[3])[m], key, "a message's parameters are a sequence of tensors", nt, &dev,
                            sz.data(), &ps[(size_t)m * nt]))
      return message_error(b, true);
  }
  // (every tensor checked: the gradient buffer is allocated now)
  at::Tensor flat;
  std::vector<at::Tensor> gv;
  if (!gradient_views(pt, sz, dev, &flat, &gv, gp.data())) return nullptr;
  float* const* ppp = p_on ? pp.data() : nullptr;
  const float* const* psp = p_on ? ps.data() : nullptr;
  const float* wpp = p_on ? wp.data() : nullptr;
  if (!on_device(dev, shape.name(kGradientForm), [&](void* st) {
        return shape.gradient(ppp, gp.data(), psp, rp.data(), wpp, wg.data(), (int)ns, n, sz.data(), (int)nt,
                              (float)inertia, st);
      }))
    return nullptr;
  return views_result(pt, gv, flat, set_grad != 0);
}
PyObject* avg_and_gradient_records(PyObject*, PyObject* args) {
  PyObject *params, *msgs, *recs, *wpar, *wgrd;
  long long n, k;
  int levels, set_grad = 0;
  double inertia;
  if (!PyArg_ParseTuple(args, "OOOOOLLid|p", &params, &msgs, &recs, &wpar, &wgrd, &n, &k, &levels, &inertia, &set_grad))
    return nullptr;
  return avg_and_gradient_records_of(stacked_shape(k, levels), params, msgs, recs, wpar, wgrd, n, inertia, set_grad);
}
// avg_and_gradient_sparse_records(params, msgs, records, w_params, w_grads, n, k, inertia, set_grad): the same for a
// round of sparse records (flc_avg_and_gradient_sparse_records; the flc_sparse_wire_layout(n, k) layout)
PyObject* avg_and_gradient_sparse_records(PyObject*, PyObject* args) {
  PyObject *params, *msgs, *recs, *wpar, *wgrd;
  long long n, k;
  int set_grad = 0;
  double inertia;
  if (!PyArg_ParseTuple(args, "OOOOOLLd|p", &params, &msgs, &recs, &wpar, &wgrd, &n, &k, &inertia, &set_grad))
    return nullptr;
  return avg_and_gradient_records_of(sparse_shape(k), params, msgs, recs, wpar, wgrd, n, inertia, set_grad);
}
// avg_and_gradient_dense_records(params, msgs, records, w_params, w_grads, n, format, levels, bits, inertia, set_grad):
// the same for a round of dense records (flc_avg_and_gradient_dense_records; the flc_dense_wire_layout(n, format, bits)
// layout of a dithering or natural-compressor message)
PyObject* avg_and_gradient_dense_records(PyObject*, PyObject* args) {
  PyObject *params, *msgs, *recs, *wpar, *wgrd;
  long long n;
  int format, levels, bits, set_grad = 0;
  double inertia;
  if (!PyArg_ParseTuple(args, "OOOOOLiiid|p", &params, &msgs, &recs, &wpar, &wgrd, &n, &format, &levels, &bits, &inertia,
                        &set_grad))
    return nullptr;
  if (format < 0) return value_error("bad wire shape");  // (before anything else is looked at)
  return avg_and_gradient_records_of(dense_shape(format, levels, bits), params, msgs, recs, wpar, wgrd, n, inertia,
                                     set_grad);
}

void release_storage(void* ctx) { delete static_cast<c10::Storage*>(ctx); }

// alias(host_tensor, device_index) -> tensor on cuda:device_index over the same bytes (see the header)
PyObject* alias(PyObject*, PyObject* args) {
  PyObject* o;
  int dev;
  if (!PyArg_ParseTuple(args, "Oi", &o, &dev)) return nullptr;
  if (!THPVariable_Check(o)) return type_error("alias takes a tensor");
  const at::Tensor& t = THPVariable_Unpack(o);
  if (!t.is_cpu() || !t.is_contiguous() || !t.is_pinned()) return type_error("alias takes a contiguous pinned host tensor");
  void* p = t.data_ptr();
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost || a.devicePointer != p) {
    (void)hipGetLastError();
    PyErr_SetString(PyExc_RuntimeError, "the pinned buffer is not mapped at its host address on the device");
    return nullptr;
  }
  const size_t nbytes = (size_t)t.numel() * t.element_size();
  auto* held = new c10::Storage(t.storage());
  c10::DataPtr dp(p, held, &release_storage, c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)dev));
  c10::Storage st(c10::Storage::use_byte_size_t(), nbytes, std::move(dp), /*allocator=*/nullptr, /*resizable=*/false);
  at::Tensor d = at::empty({0}, t.options().device(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)dev)).pinned_memory(false));
  d.set_(st, 0, t.sizes(), t.strides());
  return THPVariable_Wrap(d);
}

PyMethodDef kMethods[] = {
    {"model_fold", model_fold, METH_VARARGS,
     "model_fold(dsts, msgs, key, weights, init_mode, beta, theta, v, opt, lr, beta2, tau): flc_model_fold on Python "
     "lists of HIP tensors, launched on the current stream of the model's device"},
    {"server_fold", server_fold, METH_VARARGS,
     "server_fold(theta, aux, msgs, key, weights, kind, fold, init_mode, inertia, c): flc_model_fold_server (FedDyn / "
     "pFedMe) on Python lists of HIP tensors, at most 16 messages, on the current stream of the model's device"},
    {"avg_and_gradients", avg_and_gradients, METH_VARARGS,
     "avg_and_gradients(params, grads, msgs, w_params, w_grads, inertia[, set_grad]): flc_avg_and_gradients on Python "
     "lists of HIP "
     "tensors (messages: mappings with 'parameters' and 'gradients'), on the current stream of the model's device"},
    {"fold_records", fold_records, METH_VARARGS,
     "fold_records(records, weights, n, k, levels, delta, theta, v, beta0, opt, lr, beta2, tau): "
     "flc_fedopt_fold_records on Python lists"},
    {"fold_dense_records", fold_dense_records, METH_VARARGS,
     "fold_dense_records(records, weights, n, format, levels, bits, delta, theta, v, beta0, opt, lr, beta2, tau): "
     "flc_fedopt_fold_dense_records on Python lists"},
    {"fold_sparse_records", fold_sparse_records, METH_VARARGS,
     "fold_sparse_records(records, weights, n, k, delta, theta, v, beta0, opt, lr, beta2, tau): "
     "flc_fedopt_fold_sparse_records on Python lists"},
    {"fold_mixed_records", fold_mixed_records, METH_VARARGS,
     "fold_mixed_records(records, weights, n, kinds, ks, formats, levels, bits, delta, theta, v, beta0, opt, lr, beta2, "
     "tau): flc_fedopt_fold_mixed_records on Python lists (one descriptor per record)"},
    {"fold_record_groups", fold_record_groups, METH_VARARGS,
     "fold_record_groups(records, weights, dsts, n, k, levels): flc_fold_record_groups on Python lists (one sequence "
     "per group)"},
    {"avg_and_gradient_records", avg_and_gradient_records, METH_VARARGS,
     "avg_and_gradient_records(params, msgs, records, w_params, w_grads, n, k, levels, inertia[, set_grad]): "
     "flc_avg_and_gradient_records on Python lists (messages: mappings with 'parameters', or None)"},
    {"avg_and_gradient_sparse_records", avg_and_gradient_sparse_records, METH_VARARGS,
     "avg_and_gradient_sparse_records(params, msgs, records, w_params, w_grads, n, k, inertia[, set_grad]): "
     "flc_avg_and_gradient_sparse_records on Python lists"},
    {"avg_and_gradient_dense_records", avg_and_gradient_dense_records, METH_VARARGS,
     "avg_and_gradient_dense_records(params, msgs, records, w_params, w_grads, n, format, levels, bits, inertia"
     "[, set_grad]): flc_avg_and_gradient_dense_records on Python lists"},
    {"delta_flat", delta_flat, METH_VARARGS,
     "delta_flat(local, global): a new flat fp32 tensor cat(local - global) (flc_delta_flatten) on the tensors' device"},
    {"ef_accumulate", ef_accumulate, METH_VARARGS,
     "ef_accumulate(local, global_or_None, e): e += cat(local - global) in place (flc_ef_accumulate) on the current "
     "stream of the memory's device"},
    {"stacked_records_round", stacked_records_round, METH_VARARGS,
     "stacked_records_round(flats, seeds, counters, k, levels, records, counts, ws[, order]): flc_stacked_encode_round into the "
     "rows of a record block, one Philox counter per message, the send counts written by the encode itself"},
    {"stacked_delta_record", stacked_delta_record, METH_VARARGS,
     "stacked_delta_record(local, global, k, levels, seed, counter, record, count, ws[, order]): flc_stacked_encode_delta into a "
     "packed wire record (+ flc_delta_count_nonzero_at into count) on the current stream of the tensors' device"},
    {"alias", alias, METH_VARARGS,
     "alias(host_tensor, device_index): a HIP-device tensor over a pinned host tensor's memory (zero-copy)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef kModule = {PyModuleDef_HEAD_INIT, "_flcfold", nullptr, -1, kMethods};

}  // namespace

PyMODINIT_FUNC PyInit__flcfold(void) { return PyModule_Create(&kModule); }
